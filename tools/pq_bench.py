"""What the product-quantized row store costs: k_pq_scores over random codes, the encode rate, the whole host call,
and IndexFlat.search on fp32 rows of the same shape beside them.

    python tools/pq_bench.py [--shapes 100000x768,10000000x768,100000x8192] [--iters 10] [--json profiles/pq.json]

Per shape and nq in (1, 16, 1000): the kernel time of k_pq_scores per search (all its passes of 16 queries; the
library's own event timing, css_prof_*, around the launches of search_dev on device-resident queries) as the range over
--rounds rounds that ALTERNATE with the flat search, the code bytes per pass over the time of a pass against --hbm-gbs,
the codebook bytes a pass re-reads from L2 (grid x 4096 M, from the row tile the launcher picks), and the whole host
call (upload, launches, copies back, one wait; host clock, median of 3 after a warm-up).  The codes are random bytes
(add_codes): the scan does not care, and 10 M fp32 rows would be 30 GB of host memory.  The encode rate is one add_dev
of --encode-rows device-resident Gaussian rows, timed with a synchronise.  The flat index is filled the same way and
is skipped above --flat-max-rows rows.  No threshold: there is no predecessor."""
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
from claude_semantic_search_amd.flat_index import IndexFlatIP  # noqa: E402
from claude_semantic_search_amd.pq import IndexPQ, ProductQuantizer  # noqa: E402


def row_tile(n: int, cus: int) -> int:
    """The launcher's choice (pq_search_enqueue): the largest 256 G, G in (8, 4, 2), that gives every CU two blocks."""
    for g in (8, 4, 2):
        if -(-n // (256 * g)) >= 2 * cus:
            return 256 * g
    return 256


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x768,10000000x768,100000x8192")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--encode-rows", type=int, default=100000)
    ap.add_argument("--flat-max-rows", type=int, default=1000000)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "pq.json"))
    a = ap.parse_args()
    import torch

    assert nat.device_count() > 0, "pq_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"iters": a.iters, "rounds": a.rounds, "cus": cus, "shapes": []}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        M = d // 8
        rng = np.random.default_rng(d + n % 1000)
        pq = ProductQuantizer(d, rng.standard_normal((M, 256, 8)).astype(np.float32))
        ix = IndexPQ(d, pq)
        for r0 in range(0, n, 1 << 20):
            ix.add_codes(rng.integers(0, 256, size=(min(1 << 20, n - r0), M), dtype=np.uint8))
        flat = None
        if n <= a.flat_max_rows:
            flat = IndexFlatIP(d)
            for r0 in range(0, n, 1 << 16):
                x = torch.randn((min(1 << 16, n - r0), d), dtype=torch.float32, device=dev)
                flat.add_dev(x.data_ptr(), x.shape[0], stream=torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
        tile = row_tile(n, cus)
        grid = -(-n // tile)
        row = {"n": n, "d": d, "M": M, "code_bytes": n * M, "row_tile": tile, "grid": grid,
               "codebook_reread_bytes_per_pass": grid * 4096 * M, "queries": []}
        for nq in (1, 16, 1000):
            q = rng.standard_normal((nq, d)).astype(np.float32)
            qd = torch.from_numpy(q).to(dev)
            passes = -(-nq // 16)
            ix.search_dev(qd, 10)   # warm-up
            if flat is not None:
                flat.search(q, 10)
            torch.cuda.synchronize()
            kern, flat_ms = [], []
            for _ in range(a.rounds):   # the two alternate
                nat.prof_reset()
                nat.prof_enable(True)
                for _ in range(a.iters):
                    ix.search_dev(qd, 10)
                torch.cuda.synchronize()
                kern.append(nat.prof_read("pq_scores")[0] / a.iters)
                nat.prof_enable(False)
                if flat is not None:
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        flat.search(q, 10)
                    flat_ms.append((time.perf_counter() - t0) * 1e3 / a.iters)
            calls = []
            for _ in range(3):
                t0 = time.perf_counter()
                ix.search(q, 10)
                calls.append((time.perf_counter() - t0) * 1e3)
            best = min(kern) / passes
            row["queries"].append({
                "nq": nq, "passes": passes, "pq_scores_ms_per_search_range": [min(kern), max(kern)],
                "pq_scores_ms_per_pass_best": best, "code_gbs_per_pass": n * M / best / 1e6,
                "share_of_hbm": n * M / best / 1e6 / a.hbm_gbs, "codebook_reread_gbs": grid * 4096 * M / best / 1e6,
                "score_column_bytes_per_pass": min(nq, 16) * n * 4,
                "host_call_ms_median_of_3_warm": float(np.median(calls)),
                "flat_search_host_call_ms_range": [min(flat_ms), max(flat_ms)] if flat_ms else None})
        m = min(a.encode_rows, n)
        with IndexPQ(d, pq) as enc:
            x = torch.randn((m, d), dtype=torch.float32, device=dev)
            enc.add_dev(x[:1024].contiguous())   # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc.add_dev(x)
            torch.cuda.synchronize()
            row["encode"] = {"rows": m, "ms": (time.perf_counter() - t0) * 1e3}
            row["encode"]["rows_per_s"] = m / row["encode"]["ms"] * 1e3
        ix.close()
        if flat is not None:
            flat.close()
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
