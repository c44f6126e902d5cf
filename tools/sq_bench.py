"""What the scalar-quantized row store costs: k_sq_topk (scan and selection in one kernel) over random codes at 4 and 8
bits, the part merge beside it and the whole host call; in the same run the asymmetric search of the binary store and
IndexFlat.search on the same shapes.

    python tools/sq_bench.py [--shapes 100000x768,10000000x768] [--iters 10] [--rounds 5] [--json profiles/sq.json]

Per shape, bit width and nq in (1, 16, 1000), k = 10: the kernel time of k_sq_topk and of the merge per search (all passes
of 16 queries; the library's own event timing, css_prof_*, around the launches of search_i8_dev on device-resident int8
queries) as the range over --rounds rounds, the code bytes per pass over the best time of a pass against --hbm-gbs, and
the whole host call of search_i8 (upload, launches, copies back, one wait; host clock).  The codes are random bytes: the
scan does not care.  No threshold: there is no predecessor."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
from binary_bench import host_call_ms  # noqa: E402

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.binary import IndexBinaryFlat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from claude_semantic_search_amd.sq import IndexScalarQuantizer, ScalarQuantizer  # noqa: E402

NQS = (1, 16, 1000)


def kernel_legs(call, scan: str, merge: str, passes: int, code_bytes: int, a) -> dict:
    """Kernel times of `call` per search under the profile names `scan` and `merge`: ranges over a.rounds rounds of a.iters calls."""
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
        t_merge.append(nat.prof_read(merge)[0] / a.iters)
        nat.prof_enable(False)
    best = min(t_scan) / passes
    return {"scan_ms_per_search_range": [min(t_scan), max(t_scan)], "merge_ms_per_search_range": [min(t_merge), max(t_merge)],
            "scan_ms_per_pass_best": best, "code_bytes": code_bytes, "code_gbs_per_pass": code_bytes / best / 1e6,
            "share_of_hbm": code_bytes / best / 1e6 / a.hbm_gbs}


def fill(add, n: int, width: int, rng) -> None:
    for r0 in range(0, n, 1 << 20):
        add(rng.integers(0, 256, size=(min(1 << 20, n - r0), width), dtype=np.uint8))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x768,10000000x768")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "sq.json"))
    a = ap.parse_args()
    import torch

    assert nat.device_count() > 0, "sq_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    res = {"iters": a.iters, "rounds": a.rounds, "k": 10, "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "hbm_gbs": a.hbm_gbs, "shapes": []}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(d + n % 1000)
        q8s = {nq: rng.integers(-128, 128, size=(nq, d), dtype=np.int8) for nq in NQS}
        row = {"n": n, "d": d, "sq": [], "binary_asym": [], "flat": []}
        for bits in (4, 8):
            with IndexScalarQuantizer(ScalarQuantizer(d, bits, np.zeros(d, np.float32), np.ones(d, np.float32))) as ix:
                fill(ix.add_codes, n, ix.code_size, rng)
                for nq, q8 in q8s.items():
                    q8d, passes = torch.from_numpy(q8).to(dev), -(-nq // 16)
                    leg = kernel_legs(lambda: ix.search_i8_dev(q8d, 10), "sq_topk", "sq_merge", passes, n * ix.code_size, a)
                    leg["host_call_ms_range"] = host_call_ms(lambda: ix.search_i8(q8, 10), a.rounds)
                    row["sq"].append({"bits": bits, "nq": nq, "passes": passes, **leg})
        with IndexBinaryFlat(d) as bx:
            fill(bx.add, n, d // 8, rng)
            for nq, q8 in q8s.items():
                q8d, passes = torch.from_numpy(q8).to(dev), -(-nq // 16)
                leg = kernel_legs(lambda: bx.search_asym_i8_dev(q8d, 10), "bin_asym_topk", "bin_merge", passes, n * d // 8, a)
                row["binary_asym"].append({"nq": nq, "passes": passes, **leg})
        flat = IndexFlatIP(d)
        for r0 in range(0, n, 1 << 16):
            x = torch.randn((min(1 << 16, n - r0), d), dtype=torch.float32, device=dev)
            flat.add_dev(x.data_ptr(), x.shape[0], stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for nq in NQS:
            q = rng.standard_normal((nq, d)).astype(np.float32)
            row["flat"].append({"nq": nq, "search_host_call_ms_range": host_call_ms(lambda: flat.search(q, 10), a.rounds)})
        flat.close()
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
