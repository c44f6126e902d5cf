"""What late-interaction re-ranking costs: css_encoder_forward_maxsim against css_encoder_forward of the same batch, and
css_encoder_maxsim alone over kept token matrices, under the library's own kernel timing (css_prof_*).  Synthetic
weights, bf16 product mode, one process.

    python tools/late_bench.py [--texts 64] [--iters 20] [--docs 1000] [--doc-tokens 256] [--json profiles/late.json]
    CSS_HIP_LIB=build_ab/libcss_hip_NAME.so python tools/late_bench.py --cached-only --json ""    (a library variant)

1. One realistic re-rank batch -- `texts` sequences of 224 .. 287 tokens, one 32-token query -- at hidden 384 with 6
   layers and P = 96, and at hidden 768 with 12 layers and P = 128.  Per geometry, per call, summed over the named
   kernels: the plain forward, forward_maxsim, and the token-vector and MaxSim kernels alone.  The calls alternate.
2. MaxSim alone over `docs` kept matrices of `doc-tokens` tokens at P = 128 and P = 768, one 32-token query: the kernel
   time next to the time the bytes read would take at the HBM rate given by --hbm-gbs (an expectation, no threshold).
   The blocks per doc of the MaxSim launch follow from the number of pairs and CSS_MAXSIM_BLOCKS_PER_CU, a compile-time
   constant of csrc/css_encoder.hip: `tools/build_variant.sh ms8 -DCSS_MAXSIM_BLOCKS_PER_CU=8` builds a variant that
   spreads each of the 1000 docs over 3 blocks, `=16` over 5 (DESIGN.md 3.3d has the three side by side).
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
from claude_semantic_search_amd.late_interaction import f32_to_bf16, synth_projection  # noqa: E402
from claude_semantic_search_amd.mpnet_encoder import BERT_BASE_CFG, BERT_SMALL_CFG, MpnetEncoder  # noqa: E402

KERNELS = ("enc_embed_ln", "enc_gemm_qkv", "enc_attention", "enc_gemm_o", "enc_layernorm", "enc_gemm_ffn1",
           "enc_gemm_ffn2", "enc_pool", "enc_tok_vec", "enc_maxsim")


def prof(fn, iters: int) -> dict:
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fn()
    out = {k: nat.prof_read(k)[0] / iters for k in KERNELS}
    nat.prof_enable(False)
    nat.prof_reset()
    return out


def unit_rows(rng, n: int, P: int) -> np.ndarray:
    x = rng.standard_normal((n, P)).astype(np.float32)
    return f32_to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True))


def run_forward(name: str, cfg: dict, P: int, texts: int, iters: int) -> dict:
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=cfg)
    enc.set_token_projection(synth_projection(cfg["hidden"], P, 1))
    rng = np.random.default_rng(texts)
    lens = (224 + rng.integers(0, 64, size=texts)).tolist()
    batch = [[101] + rng.integers(1000, cfg["vocab"], size=n - 2).tolist() + [102] for n in lens]
    q = [unit_rows(rng, 32, P)]
    for _ in range(3):
        enc.encode_ids(batch)
        enc.score_late_ids(batch, q)
    f, m = [], []
    for _ in range(4):                      # alternating blocks: both see the same clocks
        f.append(prof(lambda: enc.encode_ids(batch), iters // 4))
        m.append(prof(lambda: enc.score_late_ids(batch, q), iters // 4))
    enc.close()
    fm = {k: float(np.median([r[k] for r in f])) for k in KERNELS}
    mm = {k: float(np.median([r[k] for r in m])) for k in KERNELS}
    tf, tm = sum(fm.values()), sum(mm.values())
    return {"what": "forward_maxsim", "geometry": name, "hidden": cfg["hidden"], "layers": cfg["num_layers"], "P": P,
            "texts": texts, "tokens": int(sum(lens)), "forward_ms": round(tf, 4), "forward_maxsim_ms": round(tm, 4),
            "maxsim_over_forward": round(tm / tf, 4), "added_ms": round(tm - tf, 4),
            "tok_vec_ms": round(mm["enc_tok_vec"], 4), "maxsim_ms": round(mm["enc_maxsim"], 4)}


def run_cached(enc: MpnetEncoder, P: int, docs: int, doc_tokens: int, iters: int, hbm_gbs: float) -> dict:
    rng = np.random.default_rng(P)
    rows = unit_rows(rng, docs * doc_tokens, P)
    d = [rows[j * doc_tokens:(j + 1) * doc_tokens] for j in range(docs)]
    q = [unit_rows(rng, 32, P)]
    for _ in range(3):
        enc.maxsim(q, d)
    t = [prof(lambda: enc.maxsim(q, d), iters // 4)["enc_maxsim"] for _ in range(4)]
    nbytes = rows.nbytes + docs * q[0].nbytes          # every doc row once, the query once per pair (L2 hits)
    return {"what": "maxsim_cached", "P": P, "docs": docs, "doc_tokens": doc_tokens, "query_tokens": 32,
            "maxsim_ms": round(float(np.median(t)), 4), "min_ms": round(float(min(t)), 4), "max_ms": round(float(max(t)), 4),
            "doc_bytes": int(rows.nbytes), "hbm_gbs_assumed": hbm_gbs, "hbm_ms": round(nbytes / (hbm_gbs * 1e9) * 1e3, 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--doc-tokens", type=int, default=256)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate for the expectation (MI355X peak: 8 TB/s)")
    ap.add_argument("--cached-only", action="store_true", help="part 2 alone (A/B of library variants, CSS_HIP_LIB)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "late.json"))
    a = ap.parse_args()
    res = []
    if not a.cached_only:
        res = [run_forward("small-6", dict(BERT_SMALL_CFG, num_layers=6, pooling="cls"), 96, a.texts, a.iters),
               run_forward("base-12", dict(BERT_BASE_CFG, num_layers=12, pooling="cls"), 128, a.texts, a.iters)]
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=dict(BERT_SMALL_CFG, num_layers=1, vocab=1000))
    res += [run_cached(enc, P, a.docs, a.doc_tokens, a.iters, a.hbm_gbs) for P in (128, 768)]
    enc.close()
    for r in res:
        print(json.dumps(r), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
