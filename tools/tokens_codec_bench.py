"""What compressed token matrices cost and what they lose: k_tok_scores on the codes (NB = nbits) next to k_tok_scores (NB = 0) over the
decoded matrices, k_tok_encode, the stored bytes, and the score error of a trained codec on clustered synthetic tokens.
The library's own kernel timing (css_prof_*), one process, the calls alternating in blocks.

    python tools/tokens_codec_bench.py [--docs 100000] [--doc-tokens 128] [--iters 20] [--json profiles/tokens_codec.json]
    python tools/tokens_codec_bench.py --scan-only 128 2      # the compressed scan alone, for a counters run of its own

Before anything is timed, per (P, nbits): the scores of 65 536 rows over the compressed store equal, in bits, those of a
second index that holds the decoded matrices (get_tokens).  Then, with `docs` docs of `doc-tokens` tokens and a 32-token
query, per P in (128, 96) and nbits in (1, 2, 4):
 (a) k_tok_scores<P, MT, NB> inside search_maxsim (scope tok_scores_c): kernel time, the bytes the layout implies (2 + P nbits / 8 per token, 16 per
     row) and the rate they give;
 (b) k_tok_scores in the same session on the second index (2 P bytes per token);
 (d) maxsim_ids for 64 ids: the kernel and the whole call;
 (e) bytes per token as stored: the device memory that set_token_codes / set_tokens took (hipMemGetInfo before and
     after; buffers grow by doubling, so this is an upper figure) next to the layout's 2 + P nbits / 8.
 (c) k_tok_encode in tokens/s at C = 4096 and C = 256 (P = 128), next to 2 C P FLOP per token at the bf16 MFMA peak
     given by --mfma-tflops.
 (f) per nbits, clustered synthetic tokens (synth.clustered_token_matrices) and a trained codec: the largest and mean
     absolute difference between compressed and uncompressed MaxSim scores and the top-10 overlap of search_maxsim.
     Reported, not asserted.  Real ColBERT checkpoints are not available offline; the tokens are synthetic.
The codes of (a) are uniform over C = 4096 centroids (a 1 MB table at P = 128): the gather sees no locality that real,
clustered tokens would give it.
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
from claude_semantic_search_amd import synth  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlat, TokenCodec  # noqa: E402

KERNELS = ("tok_scores", "tok_scores_c", "tok_encode", "sparse_topk")


def prof(fn, iters: int) -> dict:
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fn()
    out = {k: nat.prof_read(k)[0] / iters for k in KERNELS}
    nat.prof_enable(False)
    nat.prof_reset()
    return out


def wall(fn, iters: int) -> float:
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def stats(v) -> dict:
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


def free_bytes() -> int:
    import torch

    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info(0)[0])


def unit_bf16(rng, n: int, P: int) -> np.ndarray:
    x = rng.standard_normal((n, P)).astype(np.float32)
    return fi.f32_to_bf16_rne(x / np.linalg.norm(x, axis=1, keepdims=True))


def random_codec(rng, C: int, P: int, nbits: int) -> TokenCodec:
    """Unit centroids and the quantile buckets of Gaussian residuals of spread 0.25 / sqrt(P)."""
    cut, w = fi.residual_quantiles(rng.standard_normal(1 << 16).astype(np.float32) * np.float32(0.25 / np.sqrt(P)), nbits)
    return TokenCodec(fi.bf16_to_f32(unit_bf16(rng, C, P)), nbits, cut, w)


def compressed_index(rng, P: int, nbits: int, docs: int, doc_tokens: int, C: int = 4096):
    """(index over `docs` rows with random codes, offsets): a block of 10 000 docs repeated -- as many distinct
    addresses as distinct docs."""
    codec = random_codec(rng, C, P, nbits)
    block = min(docs, 10000) * doc_tokens
    reps = -(-docs * doc_tokens // block)
    codes = np.tile(rng.integers(0, C, size=block, dtype=np.uint16), reps)[:docs * doc_tokens]
    res = np.tile(rng.integers(0, 256, size=(block, codec.res_bytes), dtype=np.uint8), (reps, 1))[:docs * doc_tokens]
    off = np.arange(docs + 1, dtype=np.int64) * doc_tokens
    ix = IndexFlat(32, 0)
    ix.add_synthetic(docs, 1)
    ix.set_token_codec(codec)
    before = free_bytes()
    ix.set_token_codes(off, codes, res)
    return ix, off, before - free_bytes()


def scan(P: int, nbits: int, docs: int, doc_tokens: int, iters: int, hbm_gbs: float) -> list:
    rng = np.random.default_rng(1000 * P + nbits)
    ix, off, taken_c = compressed_index(rng, P, nbits, docs, doc_tokens)
    q = unit_bf16(rng, 32, P)
    plain = IndexFlat(32, 0)
    plain.add_synthetic(docs, 1)
    doff, dtok = ix.get_tokens()
    before = free_bytes()
    plain.set_tokens((doff, dtok, P))
    taken_p = before - free_bytes()
    del dtok
    ntok = int(off[-1])
    # the same bits before anything is timed
    ids = np.arange(min(docs, 65536))
    assert np.array_equal(ix.maxsim_ids(q, ids).view(np.uint32), plain.maxsim_ids(q, ids).view(np.uint32)), (P, nbits)
    assert np.array_equal(ix.search_maxsim(q, 128)[1], plain.search_maxsim(q, 128)[1]), (P, nbits)
    on_codes, on_tokens = (lambda: ix.search_maxsim(q, 10)), (lambda: plain.search_maxsim(q, 10))
    for _ in range(3):
        on_codes()
        on_tokens()
    a, b = [], []
    for _ in range(4):                      # alternating blocks: both see the same clocks
        a.append(prof(on_codes, max(iters // 4, 1))["tok_scores_c"])
        b.append(prof(on_tokens, max(iters // 4, 1))["tok_scores"])
    RB = P * nbits // 8
    bytes_c, bytes_p = ntok * (2 + RB) + 16 * docs, ntok * 2 * P + 16 * docs
    ta, tb = stats(a), stats(b)
    res = [{"what": "scan", "P": P, "nbits": nbits, "docs": docs, "doc_tokens": doc_tokens, "query_tokens": 32, "centroids": 4096,
            "tok_scores_c": ta, "layout_bytes": int(bytes_c), "layout_tbs": round(bytes_c / (ta["ms"] * 1e-3) / 1e12, 3),
            "hbm_ms_at_peak": round(bytes_c / (hbm_gbs * 1e9) * 1e3, 4), "tok_scores_decoded": tb, "decoded_bytes": int(bytes_p),
            "decoded_tbs": round(bytes_p / (tb["ms"] * 1e-3) / 1e12, 3), "compressed_over_decoded": round(ta["ms"] / tb["ms"], 3),
            "hbm_gbs_assumed": hbm_gbs}]
    ids64 = rng.choice(docs, size=64, replace=False).astype(np.int64)
    rows = lambda: ix.maxsim_ids(q, ids64)
    rows_p = lambda: plain.maxsim_ids(q, ids64)
    for _ in range(3):
        rows()
        rows_p()
    c, d = [], []
    for _ in range(4):
        c.append(prof(rows, iters)["tok_scores_c"])
        d.append(prof(rows_p, iters)["tok_scores"])
    res.append({"what": "maxsim_ids", "P": P, "nbits": nbits, "ids": 64, "doc_tokens": doc_tokens, "tok_scores_c": stats(c),
                "tok_scores_decoded": stats(d), "call_ms": round(wall(rows, iters), 4), "call_decoded_ms": round(wall(rows_p, iters), 4)})
    res.append({"what": "stored_bytes", "P": P, "nbits": nbits, "tokens": ntok, "layout_bytes_per_token": 2 + RB,
                "device_bytes_taken_per_token": round(taken_c / ntok, 2), "uncompressed_layout_bytes_per_token": 2 * P,
                "uncompressed_device_bytes_taken_per_token": round(taken_p / ntok, 2)})
    ix.close()
    plain.close()
    return res


def encode(C: int, P: int, ntok: int, iters: int, mfma_tflops: float) -> dict:
    rng = np.random.default_rng(C)
    codec = random_codec(rng, C, P, 2)
    tok = np.tile(unit_bf16(rng, 1 << 16, P), (-(-ntok // (1 << 16)), 1))[:ntok]
    off = np.arange(ntok + 1, dtype=np.int64)
    ix = IndexFlat(32, 0)
    ix.add_synthetic(ntok, 1)
    ix.set_token_codec(codec)
    run = lambda: ix.set_tokens((off, tok, P), row0=0)
    run()
    t = [prof(run, 1)["tok_encode"] for _ in range(max(iters // 4, 3))]
    s = stats(t)
    flop = 2.0 * C * P * ntok
    ix.close()
    return {"what": "encode", "C": C, "P": P, "nbits": 2, "tokens": ntok, "tok_encode": s,
            "tokens_per_s": round(ntok / (s["ms"] * 1e-3), 1), "tflops": round(flop / (s["ms"] * 1e-3) / 1e12, 2),
            "mfma_peak_tflops_assumed": mfma_tflops, "share_of_mfma_peak": round(flop / (s["ms"] * 1e-3) / (mfma_tflops * 1e12), 4)}


def quality(nbits: int, docs: int = 20000, P: int = 128, C: int = 1024, nq: int = 16) -> dict:
    off, tok, _ = synth.clustered_token_matrices(docs, P, 77, ncentres=512, max_len=32)
    codec = fi.train_token_codec((off, tok, P), C, nbits=nbits, niter=10, seed=1)
    plain, comp = IndexFlat(32, 0), IndexFlat(32, 0)
    for ix in (plain, comp):
        ix.add_synthetic(docs, 1)
    comp.set_token_codec(codec)
    plain.set_tokens((off, tok, P))
    comp.set_tokens((off, tok, P))
    rng = np.random.default_rng(5)
    live = np.flatnonzero(np.diff(off) > 0)
    diffs, overlap = [], []
    for j in range(nq):                     # a query: 32 tokens of one doc (repeated where it is shorter), plus noise
        r = int(rng.choice(live))
        t = fi.bf16_to_f32(tok[off[r]:off[r + 1]])
        x = t[rng.integers(0, t.shape[0], size=32)] + rng.standard_normal((32, P)).astype(np.float32) * np.float32(0.1 / np.sqrt(P))
        q = fi.f32_to_bf16_rne(x / np.linalg.norm(x, axis=1, keepdims=True))
        ids = live[:65536]
        diffs.append(np.abs(comp.maxsim_ids(q, ids).astype(np.float64) - plain.maxsim_ids(q, ids).astype(np.float64)))
        overlap.append(len(set(comp.search_maxsim(q, 10)[1][0].tolist()) & set(plain.search_maxsim(q, 10)[1][0].tolist())) / 10.0)
    d = np.concatenate(diffs)
    plain.close()
    comp.close()
    return {"what": "quality", "nbits": nbits, "P": P, "centroids": C, "docs": docs, "queries": nq, "query_tokens": 32,
            "tokens": "synthetic, clustered (512 centres, spread 0.25); no real ColBERT checkpoint offline",
            "max_abs_score_diff": round(float(d.max()), 5), "mean_abs_score_diff": round(float(d.mean()), 5),
            "top10_overlap_mean": round(float(np.mean(overlap)), 3), "top10_overlap_min": round(float(min(overlap)), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--doc-tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 96])
    ap.add_argument("--bits", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--encode-tokens", type=int, default=1 << 20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate for the expectation (MI355X peak: 8 TB/s)")
    ap.add_argument("--mfma-tflops", type=float, default=2500.0, help="bf16 MFMA peak for the expectation (MI355X: ~2.5 PF dense)")
    ap.add_argument("--scan-only", type=int, nargs=2, metavar=("P", "NBITS"), help="run the compressed scan alone (for a counters run)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "tokens_codec.json"))
    a = ap.parse_args()
    if nat.device_count() == 0:
        raise SystemExit("tokens_codec_bench needs a HIP device")
    if a.scan_only:
        P, nbits = a.scan_only
        rng = np.random.default_rng(1000 * P + nbits)
        ix, _, _ = compressed_index(rng, P, nbits, a.docs, a.doc_tokens)
        q = unit_bf16(rng, 32, P)
        for _ in range(a.iters):
            ix.search_maxsim(q, 10)
        ix.close()
        return
    res = []
    for P in a.widths:
        for nbits in a.bits:
            res += scan(P, nbits, a.docs, a.doc_tokens, a.iters, a.hbm_gbs)
            print(json.dumps(res[-3]), flush=True)
    for C in (4096, 256):
        res.append(encode(C, 128, a.encode_tokens, a.iters, a.mfma_tflops))
        print(json.dumps(res[-1]), flush=True)
    for nbits in a.bits:
        res.append(quality(nbits))
        print(json.dumps(res[-1]), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
