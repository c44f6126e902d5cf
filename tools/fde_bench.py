"""What the fixed-dimensional encoding costs: k_fde over `docs` matrices of `doc-tokens` tokens at P = 128 for
(k_sim, d_proj, reps) = (5, 16, 16) and (4, 32, 8), documents and 32-token queries.

    python tools/fde_bench.py [--docs 100000] [--doc-tokens 128] [--iters 5] [--json profiles/fde.json]

Per configuration: the kernel time (the library's own event timing, css_prof_*, around the launch of the `_dev` form on
device-resident matrices), the whole host call (upload, launch, copies back, one wait, by the host clock), the bytes the
algorithm must read and write over the kernel time against --hbm-gbs, and the matrix-core share: the least time the
sketch, the one-hot sums (bf16, --bf16-tflops) and the projection (fp32 MFMA, --fp32-tflops) could take over the
kernel time.  For scale: a float32 numpy twin of fde_numpy on a sample of the documents (this host's CPUs,
extrapolated and named so), the exhaustive search_maxsim scan of the same store, and the dense search at d = dim over
the encoded rows.  A sweep over d_proj at (4, ., 8) separates projection + store (the slope) from staging + sketch +
sums + fill (the intercept).  The host call is the median of three calls after a warm-up; add_fde is ONE cold call (it
appends).  No threshold: there is no predecessor to compare with."""
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
from claude_semantic_search_amd.late_interaction import bf16_to_f32, f32_to_bf16  # noqa: E402
from claude_semantic_search_amd.muvera import FixedDimensionalEncoding  # noqa: E402


def unit_tokens(seed: int, n: int, m: int, P: int) -> np.ndarray:
    """bf16 bits [n * m, P] of unit Gaussian rows, made in slices (the float32 image of 100 000 docs is 6.5 GB)."""
    out = np.empty((n * m, P), dtype=np.uint16)
    rng = np.random.default_rng(seed)
    for a in range(0, n * m, 1 << 20):
        x = rng.standard_normal((min(1 << 20, n * m - a), P), dtype=np.float32)
        out[a:a + x.shape[0]] = f32_to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))
    return out


def twin_f32(fde, tok: np.ndarray, m: int) -> None:
    """fde_numpy's float32 twin for equal-length documents, vectorised over the documents (numpy's threads)."""
    x = bf16_to_f32(tok).reshape(-1, m, fde.P)
    planes, proj = bf16_to_f32(fde.planes), bf16_to_f32(fde.proj)
    B = 1 << fde.k_sim
    bits = (x @ planes.T > 0).reshape(x.shape[0], m, fde.reps, fde.k_sim)
    bk = (bits << np.arange(fde.k_sim)).sum(axis=3)
    for r in range(fde.reps):
        onehot = (bk[:, :, r, None] == np.arange(B)).astype(np.float32)          # [n, m, B]
        Y = np.einsum("nmb,nmp->nbp", onehot, x)
        cnt = np.maximum(onehot.sum(axis=1), 1.0)                                  # (the fill is left out: a lower bound)
        _ = (Y @ proj[r * fde.d_proj:(r + 1) * fde.d_proj].T) / cnt[:, :, None]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--doc-tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--bf16-tflops", type=float, default=2500.0)
    ap.add_argument("--fp32-tflops", type=float, default=157.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "fde.json"))
    a = ap.parse_args()
    import torch

    assert nat.device_count() > 0, "fde_bench needs a HIP device"
    P, n, m = 128, a.docs, a.doc_tokens
    tok = unit_tokens(1, n, m, P)
    qtok = unit_tokens(2, 1024, 32, P)
    sides = {"documents": ((np.arange(n + 1, dtype=np.int64) * m, tok, P), n, m),
             "queries": ((np.arange(1025, dtype=np.int64) * 32, qtok, P), 1024, 32)}
    res = {"docs": n, "doc_tokens": m, "P": P, "iters": a.iters, "configs": []}
    for k_sim, d_proj, reps in ((5, 16, 16), (4, 32, 8)):
        fde = FixedDimensionalEncoding(P, k_sim, d_proj, reps, seed=0)
        B = 1 << k_sim
        row = {"k_sim": k_sim, "d_proj": d_proj, "reps": reps, "dim": fde.dim}
        for side, (csr, cn, cm) in sides.items():
            is_q = side == "queries"
            enc_dev = fde.encode_queries_dev if is_q else fde.encode_documents_dev
            enc_host = fde.encode_queries if is_q else fde.encode_documents
            enc_dev(csr)   # warm-up
            torch.cuda.synchronize()
            nat.prof_reset()
            nat.prof_enable(True)
            launches = a.iters * (50 if is_q else 1)   # (a query launch is 1 / 150 of a document launch)
            for _ in range(launches):
                enc_dev(csr)
            torch.cuda.synchronize()
            kernel_ms = nat.prof_read("fde")[0] / launches
            nat.prof_enable(False)
            enc_host(csr)   # warm-up: the first host call of a size allocates the encoder's device buffers
            calls = []
            for _ in range(3):
                t0 = time.perf_counter()
                enc_host(csr)
                calls.append((time.perf_counter() - t0) * 1e3)
            call_ms = float(np.median(calls))
            nbytes = cn * cm * P * 2 + cn * fde.dim * 4
            bf16_flop = cn * reps * (2.0 * cm * 16 * P + 2.0 * cm * P * max(B, 16))   # sketch (16 columns) + sums
            fp32_flop = cn * reps * 2.0 * max(B, 16) * P * d_proj                      # projection
            core_ms = (bf16_flop / (a.bf16_tflops * 1e12) + fp32_flop / (a.fp32_tflops * 1e12)) * 1e3
            row[side] = {"n": cn, "tokens": cm, "kernel_ms": kernel_ms, "host_call_ms_median_of_3_warm": call_ms,
                         "bytes": nbytes, "gbs": nbytes / kernel_ms / 1e6, "share_of_hbm": nbytes / kernel_ms / 1e6 / a.hbm_gbs,
                         "matrix_core_least_ms": core_ms, "matrix_core_share": core_ms / kernel_ms}
        sample = min(n, 2000)
        t0 = time.perf_counter()
        twin_f32(fde, tok[:sample * m], m)
        row["cpu_f32_twin_ms_extrapolated"] = (time.perf_counter() - t0) * 1e3 * n / sample
        row["cpu_f32_twin_sample_docs"] = sample
        # the same store behind an index: the exhaustive MaxSim scan, and the dense search over the encodings
        ix = IndexFlatIP(fde.dim)
        t0 = time.perf_counter()
        ix.add_fde(fde, sides["documents"][0])
        row["add_fde_ms_one_cold_call"] = (time.perf_counter() - t0) * 1e3
        q1 = qtok[:32]
        qd = fde.encode_queries([q1])
        for name, fn in (("search_maxsim_ms", lambda: ix.search_maxsim(q1, 10)), ("dense_search_nq1_ms", lambda: ix.search(qd, 10))):
            fn()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            row[name] = (time.perf_counter() - t0) * 1e3 / a.iters
        ix.close()
        fde.close()
        res["configs"].append(row)
        print(json.dumps(row), flush=True)
    # Which stage costs what: d_proj scales the projection and the store (and the bytes written) and nothing else, so the
    # slope of the document kernel time over d_proj is theirs and the intercept is staging + sketch + sums + fill.
    sweep = []
    for d_proj in (16, 32, 64):
        with FixedDimensionalEncoding(P, 4, d_proj, 8, seed=0) as fde:
            csr = sides["documents"][0]
            fde.encode_documents_dev(csr)
            torch.cuda.synchronize()
            nat.prof_reset()
            nat.prof_enable(True)
            for _ in range(a.iters):
                fde.encode_documents_dev(csr)
            torch.cuda.synchronize()
            sweep.append({"k_sim": 4, "d_proj": d_proj, "reps": 8, "kernel_ms": nat.prof_read("fde")[0] / a.iters})
            nat.prof_enable(False)
    slope = (sweep[2]["kernel_ms"] - sweep[0]["kernel_ms"]) / 48.0
    res["d_proj_sweep"] = {"points": sweep, "ms_per_d_proj": slope, "intercept_ms": sweep[0]["kernel_ms"] - 16.0 * slope}
    print(json.dumps(res["d_proj_sweep"]), flush=True)
    if a.json:
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
