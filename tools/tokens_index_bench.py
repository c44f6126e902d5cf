"""What MaxSim over the index's token matrices costs: k_tok_scores as a scan of every row, next to the existing
css_encoder_maxsim_dev over the same pairs, under the library's own kernel timing (css_prof_*), one process, the calls
alternating in blocks.

    python tools/tokens_index_bench.py [--docs 100000] [--doc-tokens 128] [--iters 20] [--json profiles/tokens_index.json]

Per P in (128, 96), one 32-token query:
 (a) k_tok_scores inside IndexFlat.search_maxsim over `docs` rows of `doc-tokens` tokens: kernel time, bytes read and
     the achieved rate next to the HBM rate given by --hbm-gbs (an expectation, no threshold);
 (b) the same (query, doc) pairs through css_encoder_maxsim_dev (k_maxsim, one block per pair) on the same bf16 rows
     held in device memory, in the same session;
 (c) IndexFlat.maxsim_ids for 64 ids: the kernel and the whole call, next to css_encoder_maxsim's kernel on 64 pairs;
 (d) search_maxsim as a whole call (upload, column, top-k, merge, copy back), k = 10 and k = 128.
The one condition is (a) <= (b).  The rows are random finite bf16 bit patterns: a block of 10 000 docs repeated, which
is as many distinct addresses as `docs` distinct docs (3.3 GB at P = 128, far beyond the 256 MB Infinity Cache).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.flat_index import IndexFlat  # noqa: E402
from claude_semantic_search_amd.mpnet_encoder import BERT_SMALL_CFG, MpnetEncoder  # noqa: E402

KERNELS = ("tok_scores", "sparse_topk", "enc_maxsim")


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


def bf16_rows(rng, n: int, P: int) -> np.ndarray:
    """Random finite bf16 bit patterns of magnitude 2^-7 .. 1, either sign."""
    return (rng.integers(0x3C00, 0x3F80, size=(n, P), dtype=np.uint16) | (rng.integers(0, 2, size=(n, P), dtype=np.uint16) << 15))


def run(enc: MpnetEncoder, P: int, docs: int, doc_tokens: int, iters: int, hbm_gbs: float) -> list:
    import torch

    rng = np.random.default_rng(P)
    block = min(docs, 10000)
    tok = np.tile(bf16_rows(rng, block * doc_tokens, P), (-(-docs // block), 1))[:docs * doc_tokens]
    off = np.arange(docs + 1, dtype=np.int64) * doc_tokens
    q = bf16_rows(rng, 32, P)
    ix = IndexFlat(32, 0)
    ix.add_synthetic(docs, 1)
    ix.set_tokens((off, tok, P))
    # (b): the same rows in device memory, every doc paired with query 0
    dev = torch.device("cuda", 0)
    d_tok = torch.from_numpy(tok.view(np.int16)).to(dev)
    cu_d = torch.from_numpy(off.astype(np.int32)).to(dev)
    q_tok = torch.from_numpy(q.view(np.int16)).to(dev)
    cu_q = torch.tensor([0, 32], dtype=torch.int32, device=dev)
    pairs = torch.stack([torch.zeros(docs, dtype=torch.int32), torch.arange(docs, dtype=torch.int32)], dim=1).contiguous().to(dev)
    scores = torch.empty(docs, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def existing():
        nat.check(nat.lib().css_encoder_maxsim_dev(enc._h, vp(q_tok), vp(cu_q), 1, vp(d_tok), vp(cu_d), docs, None, vp(pairs), docs,
                                                   P, vp(scores), ctypes.c_void_p(stream)))
        torch.cuda.synchronize()

    scan = lambda: ix.search_maxsim(q, 10)
    for _ in range(3):
        scan()
        existing()
    # the two give the same bits: what is timed is the same computation
    assert np.array_equal(ix.maxsim_ids(q, np.arange(min(docs, 65536))), scores[:65536].cpu().numpy())
    a, b = [], []
    for _ in range(4):                      # alternating blocks: both see the same clocks
        a.append(prof(scan, max(iters // 4, 1)))
        b.append(prof(existing, max(iters // 4, 1)))
    nbytes = tok.nbytes + 16 * docs
    ta, tb = stats([r["tok_scores"] for r in a]), stats([r["enc_maxsim"] for r in b])
    res = [{"what": "scan", "P": P, "docs": docs, "doc_tokens": doc_tokens, "query_tokens": 32, "bytes_read": int(nbytes),
            "tok_scores": ta, "tok_scores_tbs": round(nbytes / (ta["ms"] * 1e-3) / 1e12, 3), "hbm_gbs_assumed": hbm_gbs,
            "hbm_ms": round(nbytes / (hbm_gbs * 1e9) * 1e3, 4), "maxsim_dev": tb,
            "maxsim_dev_tbs": round(nbytes / (tb["ms"] * 1e-3) / 1e12, 3), "scan_over_existing": round(ta["ms"] / tb["ms"], 4),
            "sparse_topk_ms": round(float(np.median([r["sparse_topk"] for r in a])), 4)}]
    # (c) 64 ids against 64 pairs of the existing kernel
    ids = rng.choice(docs, size=64, replace=False).astype(np.int64)
    d64 = [tok[i * doc_tokens:(i + 1) * doc_tokens] for i in ids]
    rows = lambda: ix.maxsim_ids(q, ids)
    pair64 = lambda: enc.maxsim([q], d64)
    for _ in range(3):
        rows()
        pair64()
    c, e = [], []
    for _ in range(4):
        c.append(prof(rows, iters)["tok_scores"])
        e.append(prof(pair64, iters)["enc_maxsim"])
    res.append({"what": "maxsim_ids", "P": P, "ids": 64, "doc_tokens": doc_tokens, "tok_scores": stats(c), "maxsim_64_pairs": stats(e),
                "call_ms": round(wall(rows, iters), 4)})
    # (d) the whole search call
    res.append({"what": "search_maxsim", "P": P, "docs": docs, "doc_tokens": doc_tokens,
                "call_k10_ms": round(wall(scan, iters), 4), "call_k128_ms": round(wall(lambda: ix.search_maxsim(q, 128), iters), 4)})
    ix.close()
    del d_tok
    torch.cuda.empty_cache()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--doc-tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 96])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate for the expectation (MI355X peak: 8 TB/s)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "tokens_index.json"))
    a = ap.parse_args()
    if nat.device_count() == 0:
        raise SystemExit("tokens_index_bench needs a HIP device")
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=dict(BERT_SMALL_CFG, num_layers=1, vocab=1000))
    res = []
    for P in a.widths:
        res += run(enc, P, a.docs, a.doc_tokens, a.iters, a.hbm_gbs)
    enc.close()
    for r in res:
        print(json.dumps(r), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
