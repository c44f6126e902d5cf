"""What candidate generation buys MaxSim on the codes: search_maxsim_pruned (k_tok_ctable, k_tok_ci, the radix select,
k_tok_scores on the codes over the candidates, the top-k) next to the exhaustive search_maxsim on the same index.  The library's own
kernel timing (css_prof_*), one process, the calls alternating in four blocks of 5.

    python tools/tokens_prune_bench.py [--docs 100000] [--doc-tokens 128] [--json profiles/tokens_prune.json]
    python tools/tokens_prune_bench.py --ci-only 128 2        # the candidate stage alone, for a counters run of its own

Before anything is timed, per P: the approximate scores of 65 536 rows (maxsim_candidates under a mask of those rows)
equal, in bits, maxsim_ids of a second, uncompressed index that holds the matrices centroids[codes] of those rows, and
the candidates are the first ncand of ONE lexsort of that column.  Then, with `docs` docs of `doc-tokens` tokens, C = 4096
centroids and a 32-token query, per P in (128, 96) and nbits in (1, 2, 4):
 (a) k_tok_ctable; (b) k_tok_ci with the bytes it moves (2 per token and 16 per row from HBM, 4 x 32 per token gathered
     from the table through the caches) and the rates they give; (c) the select at ncand = 1024 / 4096 / 16 384;
 (d) the whole search_maxsim_pruned call at k = 10, next to the exhaustive k_tok_scores (scope tok_scores_c) and the whole search_maxsim call of the
     exhaustive path in the same process.
 (r) recall, reported and not asserted: synth.clustered_token_matrices, 20 000 docs, a trained codec with 1024
     centroids, 16 queries; the overlap of the pruned top-10 with the exhaustive top-10 on the same codes at
     ncand = 256 / 1024 / 4096.  Real ColBERT checkpoints are not available offline; the tokens are synthetic.
The codes of (a) to (d) are uniform over the centroids: the gather sees no locality that real tokens would give it.
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

import tokens_codec_bench as tcb  # noqa: E402
from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd import flat_index as fi  # noqa: E402
from claude_semantic_search_amd import synth  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlat  # noqa: E402

KERNELS = ("tok_ctable", "tok_ci", "tok_select", "tok_scores_c", "sparse_topk")
NCANDS = (1024, 4096, 16384)
BLOCKS, CALLS = 4, 5


def block(fn) -> dict:
    """One block of CALLS calls: kernel ms per call from css_prof_*, and the wall ms per call."""
    nat.prof_reset()
    nat.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    wall = (time.perf_counter() - t0) * 1e3 / CALLS
    out = {k: nat.prof_read(k)[0] / CALLS for k in KERNELS}
    nat.prof_enable(False)
    nat.prof_reset()
    out["call_profiled"] = wall
    return out


def wall_block(fn) -> float:
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    return (time.perf_counter() - t0) * 1e3 / CALLS


def oracle(ix, off, q, P: int, rows: int = 65536) -> None:
    """approx of `rows` rows against an uncompressed index of centroids[codes], in bits; candidates by ONE lexsort."""
    rows = min(rows, off.shape[0] - 1)
    codec = ix.get_token_codec()
    o, codes, _ = ix.get_token_codes(0, rows)
    plain = IndexFlat(32, 0)
    plain.add_synthetic(rows, 1)
    plain.set_tokens((o, fi.f32_to_bf16_rne(codec.centroids[codes]), P))
    allow = np.zeros(off.shape[0] - 1, bool)
    allow[:rows] = True
    ids, approx = ix.maxsim_candidates(q, 65536, allow=allow)
    want = plain.maxsim_ids(q, np.arange(rows))
    live = np.flatnonzero(want > -np.inf)
    assert np.array_equal(ids, live), (P, "candidate rows")
    assert np.array_equal(approx.view(np.uint32), want[live].view(np.uint32)), (P, "approx against maxsim_ids of centroids[codes]")
    for ncand in (1, 1000, 4096):
        got = ix.maxsim_candidates(q, ncand, allow=allow)
        ref = fi.maxsim_candidates_numpy(want, ncand)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), (P, ncand)
    full = ix.search_maxsim(q, 10, allow=allow)
    pr = ix.search_maxsim_pruned(q, 10, 65536, allow=allow)
    assert np.array_equal(full[1], pr[1]) and np.array_equal(full[0].view(np.uint32), pr[0].view(np.uint32)), (P, "every row a candidate")
    plain.close()


def timing(P: int, nbits: int, docs: int, doc_tokens: int, l2_tbs: float, check: bool) -> dict:
    rng = np.random.default_rng(1000 * P + nbits)
    ix, off, _ = tcb.compressed_index(rng, P, nbits, docs, doc_tokens)
    q = tcb.unit_bf16(rng, 32, P)
    if check:
        oracle(ix, off, q, P)
    ntok = int(off[-1])
    full = lambda: ix.search_maxsim(q, 10)
    pruned = {nc: (lambda nc=nc: ix.search_maxsim_pruned(q, 10, nc)) for nc in NCANDS}
    for _ in range(3):
        full()
        for fn in pruned.values():
            fn()
    prof = {"full": [], **{nc: [] for nc in NCANDS}}
    wall = {"full": [], **{nc: [] for nc in NCANDS}}
    for _ in range(BLOCKS):                  # alternating blocks: every path sees the same clocks
        prof["full"].append(block(full))
        for nc in NCANDS:
            prof[nc].append(block(pruned[nc]))
        wall["full"].append(wall_block(full))
        for nc in NCANDS:
            wall[nc].append(wall_block(pruned[nc]))
    col = lambda key, name: tcb.stats([b[name] for b in prof[key]])
    ci = col(4096, "tok_ci")
    hbm_bytes, gather_bytes = 2 * ntok + 16 * docs, 4 * 32 * ntok
    res = {"what": "pruned", "P": P, "nbits": nbits, "docs": docs, "doc_tokens": doc_tokens, "query_tokens": 32, "centroids": 4096,
           "k": 10, "tok_ctable": col(4096, "tok_ctable"), "tok_ci": ci, "tok_ci_hbm_bytes": int(hbm_bytes),
           "tok_ci_gather_bytes": int(gather_bytes), "tok_ci_gather_tbs": round(gather_bytes / (ci["ms"] * 1e-3) / 1e12, 3),
           "l2_gather_tbs_guide": l2_tbs, "tok_ci_ms_at_guide_rate": round(gather_bytes / (l2_tbs * 1e12) * 1e3, 4),
           "exhaustive": {"tok_scores_c": col("full", "tok_scores_c"), "sparse_topk": col("full", "sparse_topk"),
                          "call": tcb.stats(wall["full"])},
           "condition_call_at_4096_below_exhaustive": bool(np.median(wall[4096]) < np.median(wall["full"]))}
    for nc in NCANDS:
        res[f"ncand_{nc}"] = {"tok_select": col(nc, "tok_select"), "tok_scores_c": col(nc, "tok_scores_c"),
                              "sparse_topk": col(nc, "sparse_topk"), "call": tcb.stats(wall[nc])}
    ix.close()
    return res


def recall(docs: int = 20000, P: int = 128, C: int = 1024, nq: int = 16, nbits: int = 2) -> dict:
    off, tok, _ = synth.clustered_token_matrices(docs, P, 77, ncentres=512, max_len=32)
    codec = fi.train_token_codec((off, tok, P), C, nbits=nbits, niter=10, seed=1)
    ix = IndexFlat(32, 0)
    ix.add_synthetic(docs, 1)
    ix.set_token_codec(codec)
    ix.set_tokens((off, tok, P))
    rng = np.random.default_rng(5)
    live = np.flatnonzero(np.diff(off) > 0)
    overlap = {nc: [] for nc in (256, 1024, 4096)}
    for _ in range(nq):                      # a query: 32 tokens of one doc (repeated where it is shorter), plus noise
        r = int(rng.choice(live))
        t = fi.bf16_to_f32(tok[off[r]:off[r + 1]])
        x = t[rng.integers(0, t.shape[0], size=32)] + rng.standard_normal((32, P)).astype(np.float32) * np.float32(0.1 / np.sqrt(P))
        q = fi.f32_to_bf16_rne(x / np.linalg.norm(x, axis=1, keepdims=True))
        want = set(ix.search_maxsim(q, 10)[1][0].tolist())
        for nc in overlap:
            overlap[nc].append(len(want & set(ix.search_maxsim_pruned(q, 10, nc)[1][0].tolist())) / 10.0)
    ix.close()
    return {"what": "recall", "nbits": nbits, "P": P, "centroids": C, "docs": docs, "queries": nq, "query_tokens": 32,
            "tokens": "synthetic, clustered (512 centres, spread 0.25); no real ColBERT checkpoint offline",
            **{f"top10_overlap_ncand_{nc}": {"mean": round(float(np.mean(v)), 3), "min": round(float(min(v)), 3)}
               for nc, v in overlap.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--doc-tokens", type=int, default=128)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 96])
    ap.add_argument("--bits", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--l2-tbs", type=float, default=16.8, help="the guide's L2-served gather rate for the expectation (16.8-18.8 TB/s)")
    ap.add_argument("--ci-only", type=int, nargs=2, metavar=("P", "NBITS"), help="run maxsim_candidates alone (for a counters run)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "tokens_prune.json"))
    a = ap.parse_args()
    if nat.device_count() == 0:
        raise SystemExit("tokens_prune_bench needs a HIP device")
    if a.ci_only:
        P, nbits = a.ci_only
        rng = np.random.default_rng(1000 * P + nbits)
        ix, _, _ = tcb.compressed_index(rng, P, nbits, a.docs, a.doc_tokens)
        q = tcb.unit_bf16(rng, 32, P)
        for _ in range(20):
            ix.maxsim_candidates(q, 4096)
        ix.close()
        return
    res = []
    for P in a.widths:
        for j, nbits in enumerate(a.bits):
            res.append(timing(P, nbits, a.docs, a.doc_tokens, a.l2_tbs, check=j == 0))
            print(json.dumps(res[-1]), flush=True)
    res.append(recall())
    print(json.dumps(res[-1]), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
