"""What batching buys MaxSim search: IndexFlat.search_maxsim_batch (k_tok_scores_b: the token store read once per group of
MAXSIM_BATCH_GROUP queries) next to the loop of single search_maxsim calls over the same queries on the same index,
in ONE process, the two alternating in blocks, under the library's own kernel timing (css_prof_*) and as whole calls.

    python tools/tokens_batch_bench.py [--docs 100000] [--doc-tokens 128] [--iters 3] [--json profiles/tokens_batch.json]

Per store (raw, 2-bit codec), P in (128, 96), query length in (32, 64) and nq in (1, 2, G, 32, 256), k = 10:
 (a) first the batch is asserted equal to the loop of single calls in bytes;
 (b) whole-call time of the loop (the sum of its nq calls) and of the batch: medians and min - max over the blocks;
 (c) kernel time of the column kernels (tok_scores / tok_scores_c for the loop, tok_scores_b / tok_scores_bc plus the
     single kernel of a remainder of one for the batch), the top-k and the merge;
 (d) the batch column kernel's share of the HBM rate (--hbm-gbs) and of the bf16 matrix rate (--bf16-tflops): bytes =
     passes x the store, FLOP = 2 x 16 MT x P per stored token and query (the zero-filled tiles are multiplied too).
The condition of the feature is (b) at nq = 32, 32-token queries, P = 128: batch <= loop / 2, on either store; the
result lines carry "condition": true / false there.  The rows are random finite bf16 bit patterns (raw) or random codes
(2 bits): a block of 10 000 docs repeated, as many distinct addresses as `docs` distinct docs.
"""
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
from claude_semantic_search_amd import flat_index as fi  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlat  # noqa: E402

G = fi.MAXSIM_BATCH_GROUP
KERNELS = ("tok_scores", "tok_scores_c", "tok_scores_b", "tok_scores_bc", "sparse_topk", "knn_merge_parts")


def prof(fn, iters: int) -> dict:
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fn()
    out = {k: nat.prof_read(k)[0] / iters for k in KERNELS}
    nat.prof_enable(False)
    nat.prof_reset()
    return out


def wall(fn, iters: int) -> list:
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def stats(v) -> dict:
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


def bf16_rows(rng, n: int, P: int) -> np.ndarray:
    """Random finite bf16 bit patterns of magnitude 2^-7 .. 1, either sign."""
    return (rng.integers(0x3C00, 0x3F80, size=(n, P), dtype=np.uint16) | (rng.integers(0, 2, size=(n, P), dtype=np.uint16) << 15))


def build(rng, P: int, nbits: int, docs: int, doc_tokens: int):
    """(index, bytes of the token store): raw bf16 tokens (nbits = 0) or random codes of a random codec."""
    off = np.arange(docs + 1, dtype=np.int64) * doc_tokens
    block = min(docs, 10000) * doc_tokens
    reps = -(-docs * doc_tokens // block)
    ix = IndexFlat(32, 0)
    ix.add_synthetic(docs, 1)
    if nbits == 0:
        tok = np.tile(bf16_rows(rng, block, P), (reps, 1))[:docs * doc_tokens]
        ix.set_tokens((off, tok, P))
        return ix, tok.nbytes + 16 * docs
    C = 4096
    cut, w = fi.residual_quantiles(rng.standard_normal(1 << 16).astype(np.float32) * np.float32(0.25 / np.sqrt(P)), nbits)
    x = rng.standard_normal((C, P)).astype(np.float32)
    cent = fi.bf16_to_f32(fi.f32_to_bf16_rne(x / np.linalg.norm(x, axis=1, keepdims=True)))
    codec = fi.TokenCodec(cent, nbits, cut, w)
    ix.set_token_codec(codec)
    codes = np.tile(rng.integers(0, C, size=block, dtype=np.uint16), reps)[:docs * doc_tokens]
    res = np.tile(rng.integers(0, 256, size=(block, codec.res_bytes), dtype=np.uint8), (reps, 1))[:docs * doc_tokens]
    ix.set_token_codes(off, codes, res)
    return ix, codes.nbytes + res.nbytes + 16 * docs


def run(P: int, nbits: int, a) -> list:
    rng = np.random.default_rng(1000 * P + nbits)
    ix, store_bytes = build(rng, P, nbits, a.docs, a.doc_tokens)
    ntok = a.docs * a.doc_tokens
    single, group = ("tok_scores_c", "tok_scores_bc") if nbits else ("tok_scores", "tok_scores_b")
    out = []
    for mq in a.query_tokens:
        for nq in a.nq:
            qs = [bf16_rows(rng, mq, P) for _ in range(nq)]
            loop = lambda: [ix.search_maxsim(q, a.k) for q in qs]
            batch = lambda: ix.search_maxsim_batch(qs, a.k)
            # (a) the same bytes before anything is timed (this is the warm-up as well)
            want, got = loop(), batch()
            assert np.array_equal(np.concatenate([w[0] for w in want]).view(np.uint32), got[0].view(np.uint32)), (P, nbits, mq, nq)
            assert np.array_equal(np.concatenate([w[1] for w in want]), got[1]), (P, nbits, mq, nq)
            passes = ix.last_maxsim_passes
            assert passes == -(-nq // G)
            it = max(1, a.iters if nq <= 32 else a.iters // 2)
            wl, wb, pl, pb = [], [], [], []
            for _ in range(a.blocks):              # alternating blocks: both see the same clocks
                wl += wall(loop, it)
                wb += wall(batch, it)
                pl.append(prof(loop, it))
                pb.append(prof(batch, it))
            sl, sb = stats(wl), stats(wb)
            kl = stats([r[single] for r in pl])
            kb = stats([r[group] + r[single] for r in pb])
            grouped = stats([r[group] for r in pb])
            rec = {"store": f"{nbits} bits" if nbits else "raw", "P": P, "docs": a.docs, "doc_tokens": a.doc_tokens, "query_tokens": mq,
                   "nq": nq, "k": a.k, "group": G, "passes": passes, "loop_call": sl, "batch_call": sb,
                   "batch_over_loop": round(sb["ms"] / sl["ms"], 4), "loop_column_kernels": kl, "batch_column_kernels": kb,
                   "loop_topk_ms": round(float(np.median([r["sparse_topk"] for r in pl])), 4),
                   "batch_topk_ms": round(float(np.median([r["sparse_topk"] for r in pb])), 4),
                   "loop_merge_ms": round(float(np.median([r["knn_merge_parts"] for r in pl])), 4),
                   "batch_merge_ms": round(float(np.median([r["knn_merge_parts"] for r in pb])), 4)}
            full = nq // G + (1 if nq % G > 1 else 0)          # launches of the group kernel
            if full and grouped["ms"] > 0:
                sec = grouped["ms"] * 1e-3
                slots = nq - (1 if nq % G == 1 else 0)
                flop = 2.0 * 16 * ((mq + 15) // 16) * P * ntok * slots
                rec["group_kernel"] = grouped
                rec["group_kernel_hbm_share"] = round(full * store_bytes / sec / (a.hbm_gbs * 1e9), 4)
                rec["group_kernel_bf16_share"] = round(flop / sec / (a.bf16_tflops * 1e12), 4)
            if nq == 32 and mq == 32 and P == 128:
                rec["condition"] = bool(sb["ms"] <= 0.5 * sl["ms"])
            print(json.dumps(rec), flush=True)
            out.append(rec)
    ix.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--doc-tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 96])
    ap.add_argument("--bits", type=int, nargs="+", default=[0, 2], help="0: the raw store")
    ap.add_argument("--query-tokens", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 2, G, 32, 256])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate for the share (MI355X peak: 8 TB/s)")
    ap.add_argument("--bf16-tflops", type=float, default=2500.0, help="dense bf16 matrix rate for the share (MI355X: 2.5 PFLOP/s)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "tokens_batch.json"))
    a = ap.parse_args()
    if nat.device_count() == 0:
        raise SystemExit("tokens_batch_bench needs a HIP device")
    res = []
    for nbits in a.bits:
        for P in a.widths:
            res += run(P, nbits, a)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
