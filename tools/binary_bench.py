"""What the binary row store costs: k_bin_topk (scan and selection in one kernel) over random codes, the part merge
beside it and the whole host call; for one query at the first shape, IndexFlat.search and IndexPQ.search beside them.

    python tools/binary_bench.py [--shapes 100000x768,10000000x768] [--iters 10] [--json profiles/binary.json]
                                 [--asym-json profiles/binary_asym.json]

Per shape and nq in (1, 16, 1000), k = 10: the kernel time of k_bin_topk and of k_bin_merge per search (all passes of 16
queries; the library's own event timing, css_prof_*, around the launches of search_codes_dev on device-resident query
codes) as the range over --rounds rounds, the code bytes per pass over the best time of a pass against --hbm-gbs, and the
whole host call (upload, launches, copies back, one wait; host clock, range over --rounds after a warm-up).  The codes
are random bytes: the scan does not care.  No threshold: there is no predecessor.

The asymmetric search (search_asym_i8_dev, k_bin_asym_topk) is measured the same way at the same shapes and nq, on
uniform int8 queries, next to the Hamming legs of the same run; its records go to --asym-json."""
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


def scan_legs(call, scan: str, passes: int, code_bytes: int, a) -> dict:
    """Kernel times of `call` per search: the scan `scan` and bin_merge, ranges over a.rounds rounds of a.iters calls."""
    import torch

    call()   # warm-up
    torch.cuda.synchronize()
    t_scan, t_merge = [], []
    for _ in range(a.rounds):
        nat.prof_reset()
        nat.prof_enable(True)
        for _ in range(a.iters):
            call()
        torch.cuda.synchronize()
        t_scan.append(nat.prof_read(scan)[0] / a.iters)
        t_merge.append(nat.prof_read("bin_merge")[0] / a.iters)
        nat.prof_enable(False)
    best = min(t_scan) / passes
    return {f"{scan}_ms_per_search_range": [min(t_scan), max(t_scan)], "bin_merge_ms_per_search_range": [min(t_merge), max(t_merge)],
            f"{scan}_ms_per_pass_best": best, "code_gbs_per_pass": code_bytes / best / 1e6,
            "share_of_hbm": code_bytes / best / 1e6 / a.hbm_gbs}


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
    ap.add_argument("--asym-json", default=str(ROOT / "profiles" / "binary_asym.json"))
    a = ap.parse_args()
    import torch

    assert nat.device_count() > 0, "binary_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    res = {"iters": a.iters, "rounds": a.rounds, "k": 10, "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "shapes": []}
    ares = {**res, "shapes": []}
    for si, shape in enumerate(a.shapes.split(",")):
        n, d = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(d + n % 1000)
        row = {"n": n, "d": d, "code_bytes": n * d // 8, "queries": []}
        arow = {"n": n, "d": d, "code_bytes": n * d // 8, "queries": []}
        with IndexBinaryFlat(d) as ix:
            for r0 in range(0, n, 1 << 20):
                ix.add(rng.integers(0, 256, size=(min(1 << 20, n - r0), d // 8), dtype=np.uint8))
            for nq in (1, 16, 1000):
                qc = rng.integers(0, 256, size=(nq, d // 8), dtype=np.uint8)
                qd = torch.from_numpy(qc).to(dev)
                passes = -(-nq // 16)
                ham = scan_legs(lambda: ix.search_codes_dev(qd, 10), "bin_topk", passes, row["code_bytes"], a)
                ham["host_call_ms_range"] = host_call_ms(lambda: ix.search(qc, 10), a.rounds)
                row["queries"].append({"nq": nq, "passes": passes, **ham})
                # the asymmetric search of int8 queries over the same codes, in the same run
                q8 = rng.integers(-128, 128, size=(nq, d), dtype=np.int8)
                q8d = torch.from_numpy(q8).to(dev)
                asym = scan_legs(lambda: ix.search_asym_i8_dev(q8d, 10), "bin_asym_topk", passes, row["code_bytes"], a)
                asym["host_call_ms_range"] = host_call_ms(lambda: ix.search_asym(q8, 10), a.rounds)
                asym["pass_ms_over_hamming_pass_ms"] = asym["bin_asym_topk_ms_per_pass_best"] / ham["bin_topk_ms_per_pass_best"]
                arow["queries"].append({"nq": nq, "passes": passes, **asym, "hamming_same_run": ham})
        if si == 0:
            row["one_query_neighbours"] = neighbours(n, d, rng, a.rounds)
        res["shapes"].append(row)
        ares["shapes"].append(arow)
        print(json.dumps(row), flush=True)
        print(json.dumps(arow), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    if a.asym_json:
        Path(a.asym_json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.asym_json).write_text(json.dumps(ares, indent=1) + "\n")


if __name__ == "__main__":
    main()
