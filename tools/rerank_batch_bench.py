"""What fusing buys the two-stage search: IndexFlat.search_rerank_maxsim (the dense pool search, k_tok_scores_l over the
pool lists of ALL queries in one launch, the ranking and the outputs on the device, one upload and one wait) next to the
two ways of composing it from single calls on the same index, in ONE process, alternating in blocks, as whole calls
and under the library's own kernel timing (css_prof_*).

    python tools/rerank_batch_bench.py [--docs 100000] [--dim 768] [--doc-tokens 128] [--json profiles/rerank_batch.json]

Per store (raw, 2-bit codec) at P = 128, 32-token queries, k = 10, fetch in (64, 128) and nq in (1, 8, 64, 1000):
 first the fused call is asserted equal in bytes to the composition of search(Q, fetch) and the loop of maxsim_ids;
 (a) the fused call;
 (b) the loop of single search + maxsim_ids + host ranking, what HybridStorage.search_late_reranked does per query;
 (c) one batched search(Q, fetch), then the loop of maxsim_ids (timed apart: "search" and "loop_c_maxsim");
 the re-rank stage alone under css_prof events: rr_lists + tok_scores_l + rr_topk + rr_out for (a), tok_scores of the
 nq launches for (c).
Legs (b) and (c) run only kernels that the fused call does not touch.  Conditions: at nq >= 8 the fused call's time
behind the pool search (a - search) is below the loop of maxsim_ids calls of leg (c); at nq = 1 the fused call does not
exceed leg (b) by more than the min - max spread of (b)'s blocks.  The list kernel's share of the HBM rate (--hbm-gbs)
for the bytes of the listed rows and of the bf16 matrix rate (--bf16-tflops) are written beside the same figures of
k_tok_scores through its row list (leg (c)) at the same shape.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd import flat_index as fi  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlat  # noqa: E402
from tokens_batch_bench import bf16_rows, stats, wall  # noqa: E402

STAGE = ("rr_lists", "tok_scores_l", "tok_scores_lc", "rr_topk", "rr_out")
SINGLE = ("tok_scores", "tok_scores_c")


def prof(fn, iters: int, names) -> dict:
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fn()
    out = {k: nat.prof_read(k)[0] / iters for k in names}
    nat.prof_enable(False)
    nat.prof_reset()
    return out


def build(rng, a, nbits: int):
    """(index, bytes of one stored token): a.docs rows of a.dim with a.doc_tokens tokens each, raw or coded."""
    P, docs, doc_tokens = a.P, a.docs, a.doc_tokens
    off = np.arange(docs + 1, dtype=np.int64) * doc_tokens
    block = min(docs, 10000) * doc_tokens
    reps = -(-docs * doc_tokens // block)
    ix = IndexFlat(a.dim, 0)
    ix.add_synthetic(docs, 1)
    if nbits == 0:
        ix.set_tokens((off, np.tile(bf16_rows(rng, block, P), (reps, 1))[:docs * doc_tokens], P))
        return ix, 2 * P
    C = 4096
    cut, w = fi.residual_quantiles(rng.standard_normal(1 << 16).astype(np.float32) * np.float32(0.25 / np.sqrt(P)), nbits)
    x = rng.standard_normal((C, P)).astype(np.float32)
    codec = fi.TokenCodec(fi.bf16_to_f32(fi.f32_to_bf16_rne(x / np.linalg.norm(x, axis=1, keepdims=True))), nbits, cut, w)
    ix.set_token_codec(codec)
    codes = np.tile(rng.integers(0, C, size=block, dtype=np.uint16), reps)[:docs * doc_tokens]
    res = np.tile(rng.integers(0, 256, size=(block, codec.res_bytes), dtype=np.uint8), (reps, 1))[:docs * doc_tokens]
    ix.set_token_codes(off, codes, res)
    return ix, 2 + codec.res_bytes


def run(nbits: int, a) -> list:
    rng = np.random.default_rng(77 + nbits)
    ix, token_bytes = build(rng, a, nbits)
    lists, single = ("tok_scores_lc", "tok_scores_c") if nbits else ("tok_scores_l", "tok_scores")
    out = []
    for fetch in a.fetch:
        for nq in a.nq:
            Q = rng.standard_normal((nq, a.dim)).astype(np.float32)
            qs = [bf16_rows(rng, a.query_tokens, a.P) for _ in range(nq)]
            k = a.k

            def fused():
                return ix.search_rerank_maxsim(Q, qs, k, fetch, normalize=True)

            def search():
                return ix.search(Q, fetch, normalize=True)

            def loop_b():
                res = []
                for i in range(nq):
                    S0, I0 = ix.search(Q[i:i + 1], fetch, normalize=True)
                    sc = ix.maxsim_ids(qs[i], I0[0])
                    res.append(np.argsort(-sc, kind="stable")[:k])
                return res

            S0, I0 = search()

            def loop_c_maxsim():
                return [ix.maxsim_ids(qs[i], I0[i]) for i in range(nq)]

            # the same bytes before anything is timed (this is the warm-up as well)
            want = fi.search_rerank_maxsim_numpy(S0, I0, np.stack(loop_c_maxsim()), k)
            got = fused()
            for g, w_ in zip(got, want):
                assert g.dtype == w_.dtype and np.array_equal(g.view(np.uint8), w_.view(np.uint8)), (nbits, fetch, nq)
            loop_b()
            it = 1 if nq >= 64 else a.iters
            wa, wb, ws, wc, pa, pc = [], [], [], [], [], []
            for _ in range(a.blocks):              # alternating blocks: all legs see the same clocks
                wa += wall(fused, it)
                wb += wall(loop_b, it)
                ws += wall(search, it)
                wc += wall(loop_c_maxsim, it)
                pa.append(prof(fused, it, STAGE))
                pc.append(prof(loop_c_maxsim, it, SINGLE))
            sa, sb, ss, sc_ = stats(wa), stats(wb), stats(ws), stats(wc)
            stage = stats([sum(r.values()) for r in pa])
            klist = stats([r[lists] for r in pa])
            kloop = stats([r[single] for r in pc])
            behind = round(sa["ms"] - ss["ms"], 4)
            tokens = float(nq) * fetch * a.doc_tokens
            flop = 2.0 * 16 * ((a.query_tokens + 15) // 16) * a.P * tokens
            rate = lambda ms: (round(tokens * token_bytes / (ms * 1e-3) / (a.hbm_gbs * 1e9), 4),
                               round(flop / (ms * 1e-3) / (a.bf16_tflops * 1e12), 4)) if ms > 0 else (None, None)
            rec = {"store": f"{nbits} bits" if nbits else "raw", "P": a.P, "docs": a.docs, "dim": a.dim, "doc_tokens": a.doc_tokens,
                   "query_tokens": a.query_tokens, "nq": nq, "k": k, "fetch": fetch,
                   "a_fused_call": sa, "b_loop_of_single_calls": sb, "c_search": ss, "c_loop_of_maxsim_ids": sc_,
                   "fused_behind_search_ms": behind, "fused_over_b": round(sa["ms"] / sb["ms"], 4),
                   "fused_over_c": round(sa["ms"] / (ss["ms"] + sc_["ms"]), 4),
                   "rerank_stage_kernels": stage, "list_kernel": klist, "loop_c_kernels": kloop,
                   "list_kernel_hbm_share": rate(klist["ms"])[0], "list_kernel_bf16_share": rate(klist["ms"])[1],
                   "rows_path_hbm_share": rate(kloop["ms"])[0], "rows_path_bf16_share": rate(kloop["ms"])[1]}
            if nq >= 8:
                rec["condition"] = bool(behind < sc_["ms"])
            if nq == 1:
                rec["condition"] = bool(sa["ms"] <= sb["ms"] + (sb["max_ms"] - sb["min_ms"]))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    ix.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--doc-tokens", type=int, default=128)
    ap.add_argument("--P", type=int, default=128)
    ap.add_argument("--query-tokens", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--bits", type=int, nargs="+", default=[0, 2], help="0: the raw store")
    ap.add_argument("--fetch", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 64, 1000])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate for the share (MI355X peak: 8 TB/s)")
    ap.add_argument("--bf16-tflops", type=float, default=2500.0, help="dense bf16 matrix rate for the share (MI355X: 2.5 PFLOP/s)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "rerank_batch.json"))
    a = ap.parse_args()
    if nat.device_count() == 0:
        raise SystemExit("rerank_batch_bench needs a HIP device")
    res = []
    for nbits in a.bits:
        res += run(nbits, a)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
