"""What the binary row store costs: k_bin_topk (scan and selection in one kernel) over random codes, the part merge
beside it and the whole host call; for one query at the first shape, IndexFlat.search and IndexPQ.search beside them.

    python tools/binary_bench.py [--shapes 100000x768,10000000x768] [--iters 10] [--json profiles/binary.json]

Per shape and nq in (1, 16, 1000), k = 10: the kernel time of k_bin_topk and of k_bin_merge per search (all passes of 16
queries; the library's own event timing, css_prof_*, around the launches of search_codes_dev on device-resident query
codes) as the range over --rounds rounds, the code bytes per pass over the best time of a pass against --hbm-gbs, and the
whole host call (upload, launches, copies back, one wait; host clock, range over --rounds after a warm-up).  The codes
are random bytes: the scan does not care.  No threshold: there is no predecessor."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.binary import IndexBinaryFlat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from claude_semantic_search_amd.pq import IndexPQ, ProductQuantizer  # noqa: E402


def host_call_ms(fn, rounds: int):
    fn()   # warm-up
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return [min(ms), max(ms)]


def neighbours(n: int, d: int, rng, rounds: int) -> dict:
    """One query, k = 10, over n rows of d: the host calls of the flat index (fp32 rows) and of the PQ store."""
    import torch

    q = rng.standard_normal((1, d)).astype(np.float32)
    out = {}
    flat = IndexFlatIP(d)
    for r0 in range(0, n, 1 << 16):
        x = torch.randn((min(1 << 16, n - r0), d), dtype=torch.float32, device="cuda:0")
        flat.add_dev(x.data_ptr(), x.shape[0], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out["flat_search_host_call_ms_range"] = host_call_ms(lambda: flat.search(q, 10), rounds)
    flat.close()
    with IndexPQ(d, ProductQuantizer(d, rng.standard_normal((d // 8, 256, 8)).astype(np.float32))) as pq:
        pq.add_codes(rng.integers(0, 256, size=(n, d // 8), dtype=np.uint8))
        out["pq_search_host_call_ms_range"] = host_call_ms(lambda: pq.search(q, 10), rounds)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x768,10000000x768")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "binary.json"))
    a = ap.parse_args()
    import torch

    assert nat.device_count() > 0, "binary_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    res = {"iters": a.iters, "rounds": a.rounds, "k": 10, "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "shapes": []}
    for si, shape in enumerate(a.shapes.split(",")):
        n, d = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(d + n % 1000)
        row = {"n": n, "d": d, "code_bytes": n * d // 8, "queries": []}
        with IndexBinaryFlat(d) as ix:
            for r0 in range(0, n, 1 << 20):
                ix.add(rng.integers(0, 256, size=(min(1 << 20, n - r0), d // 8), dtype=np.uint8))
            for nq in (1, 16, 1000):
                qc = rng.integers(0, 256, size=(nq, d // 8), dtype=np.uint8)
                qd = torch.from_numpy(qc).to(dev)
                passes = -(-nq // 16)
                ix.search_codes_dev(qd, 10)   # warm-up
                torch.cuda.synchronize()
                scan, merge = [], []
                for _ in range(a.rounds):
                    nat.prof_reset()
                    nat.prof_enable(True)
                    for _ in range(a.iters):
                        ix.search_codes_dev(qd, 10)
                    torch.cuda.synchronize()
                    scan.append(nat.prof_read("bin_topk")[0] / a.iters)
                    merge.append(nat.prof_read("bin_merge")[0] / a.iters)
                    nat.prof_enable(False)
                best = min(scan) / passes
                row["queries"].append({
                    "nq": nq, "passes": passes, "bin_topk_ms_per_search_range": [min(scan), max(scan)],
                    "bin_merge_ms_per_search_range": [min(merge), max(merge)], "bin_topk_ms_per_pass_best": best,
                    "code_gbs_per_pass": row["code_bytes"] / best / 1e6,
                    "share_of_hbm": row["code_bytes"] / best / 1e6 / a.hbm_gbs,
                    "host_call_ms_range": host_call_ms(lambda: ix.search(qc, 10), a.rounds)})
        if si == 0:
            row["one_query_neighbours"] = neighbours(n, d, rng, a.rounds)
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
