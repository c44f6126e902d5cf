"""What the cross-encoder pair path adds to a forward pass: css_encoder_forward_pairs against css_encoder_forward of the
same batch, under the library's own kernel timing (css_prof_*).  Synthetic weights, bf16 product mode, one process.

    python tools/rerank_bench.py [--pairs 64] [--seq 256] [--iters 20] [--json profiles/rerank.json]

One realistic re-rank batch -- `pairs` sequences of about `seq` tokens (lengths seq - 32 .. seq + 31, segment start at
a 12-token query) -- at hidden 384 with 6 layers (ms-marco-MiniLM-L-6 geometry) and at hidden 768 with 12 layers.  Per
geometry, per call, summed over the named kernels: the plain forward, the pair forward, the embedding kernel in both
(the segment add), the head kernel, and the CLS pooling in place of the model's own pooling.  The calls alternate.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.cross_encoder import synth_head  # noqa: E402
from claude_semantic_search_amd.mpnet_encoder import BERT_BASE_CFG, BERT_SMALL_CFG, MpnetEncoder  # noqa: E402

KERNELS = ("enc_embed_ln", "enc_gemm_qkv", "enc_attention", "enc_gemm_o", "enc_layernorm", "enc_gemm_ffn1",
           "enc_gemm_ffn2", "enc_pool", "enc_ce_head")


def prof(fn, iters: int) -> dict:
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fn()
    out = {k: nat.prof_read(k)[0] / iters for k in KERNELS}
    nat.prof_enable(False)
    nat.prof_reset()
    return out


def run(name: str, cfg: dict, pairs: int, seq: int, iters: int) -> dict:
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=cfg)
    h = synth_head(cfg["hidden"], 1)
    enc.set_head(h["pooler_w"], h["pooler_b"], h["cls_w"], h["cls_b"])
    rng = np.random.default_rng(pairs)
    lens = (seq - 32 + rng.integers(0, 64, size=pairs)).tolist()
    batch = [[101] + rng.integers(1000, cfg["vocab"], size=n - 2).tolist() + [102] for n in lens]
    seg = [14] * pairs
    for _ in range(3):
        enc.encode_ids(batch)
        enc.score_pair_ids(batch, seg)
    f, p = [], []
    for _ in range(4):                      # alternating blocks: both see the same clocks
        f.append(prof(lambda: enc.encode_ids(batch), iters // 4))
        p.append(prof(lambda: enc.score_pair_ids(batch, seg), iters // 4))
    enc.close()
    fm = {k: float(np.median([r[k] for r in f])) for k in KERNELS}
    pm = {k: float(np.median([r[k] for r in p])) for k in KERNELS}
    tf, tp = sum(fm.values()), sum(pm.values())
    return {"geometry": name, "hidden": cfg["hidden"], "layers": cfg["num_layers"], "pairs": pairs, "tokens": int(sum(lens)),
            "forward_ms": round(tf, 4), "forward_pairs_ms": round(tp, 4), "pairs_over_forward": round(tp / tf, 4),
            "added_ms": round(tp - tf, 4), "embed_forward_ms": round(fm["enc_embed_ln"], 4),
            "embed_pairs_ms": round(pm["enc_embed_ln"], 4), "pool_forward_ms": round(fm["enc_pool"], 4),
            "pool_pairs_ms": round(pm["enc_pool"], 4), "ce_head_ms": round(pm["enc_ce_head"], 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "rerank.json"))
    a = ap.parse_args()
    res = [run("small-6", dict(BERT_SMALL_CFG, num_layers=6, pooling="cls", normalize=False), a.pairs, a.seq, a.iters),
           run("base-12", dict(BERT_BASE_CFG, num_layers=12, pooling="cls", normalize=False), a.pairs, a.seq, a.iters)]
    for r in res:
        print(json.dumps(r), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
