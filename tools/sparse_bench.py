"""What learned sparse encoding costs: css_encoder_forward_sparse against css_encoder_forward of the same batch, and the
vocabulary-max kernel's rate next to the FFN1 GEMM of the same session, under the library's own kernel timing
(css_prof_*).  Synthetic weights, bf16 product mode, one process.

    python tools/sparse_bench.py [--texts 64] [--iters 20] [--full] [--json profiles/sparse.json]

Per geometry (hidden 384 with 6 layers, hidden 768 with 12 layers; V = 30522, m = 256) and batch (`texts` sequences of
224 .. 287 tokens; with --full also 256 sequences of 384 tokens), per call, summed over the named kernels: the plain
forward and forward_sparse, the calls alternating in blocks; the ratio next to the one the FLOP counts alone would give
(per token: forward 2 L (4 H^2 + 2 H F) + attention 4 L H T_seq, head 2 H^2 + 2 H V); the vocabulary-max kernel's
TFLOP/s (2 T H V / t) next to FFN1's (2 T H F / t per layer); the top-m kernel's time.
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
from claude_semantic_search_amd.mpnet_encoder import BERT_BASE_CFG, BERT_SMALL_CFG, MpnetEncoder  # noqa: E402
from claude_semantic_search_amd.sparse_encoder import synth_mlm_head  # noqa: E402

KERNELS = ("enc_embed_ln", "enc_gemm_qkv", "enc_attention", "enc_gemm_o", "enc_layernorm", "enc_gemm_ffn1",
           "enc_gemm_ffn2", "enc_pool", "enc_mlm_rows", "enc_mlm_dense", "enc_mlm_ln", "enc_vocab_max", "enc_vocab_topm")
M = 256


def prof(fn, iters: int) -> dict:
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fn()
    out = {k: nat.prof_read(k)[0] / iters for k in KERNELS}
    nat.prof_enable(False)
    nat.prof_reset()
    return out


def run(name: str, cfg: dict, lens, iters: int) -> dict:
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=cfg)
    enc.set_mlm_head(**synth_mlm_head(cfg["hidden"], cfg["vocab"], 1))
    rng = np.random.default_rng(len(lens))
    batch = [[101] + rng.integers(1000, cfg["vocab"], size=n - 2).tolist() + [102] for n in lens]
    for _ in range(2):
        enc.encode_ids(batch)
        enc.encode_sparse_ids(batch, M)
    f, s = [], []
    for _ in range(4):                      # alternating blocks: both see the same clocks
        f.append(prof(lambda: enc.encode_ids(batch), max(1, iters // 4)))
        s.append(prof(lambda: enc.encode_sparse_ids(batch, M), max(1, iters // 4)))
    enc.close()
    tf = [sum(r.values()) for r in f]
    ts = [sum(r.values()) for r in s]
    med = {k: float(np.median([r[k] for r in s])) for k in KERNELS}
    T, H, F, L, V = int(sum(lens)), cfg["hidden"], cfg["ffn"], cfg["num_layers"], cfg["vocab"]
    fl_fwd = T * L * 2 * (4 * H * H + 2 * H * F) + sum(4 * L * H * n * n for n in lens)
    fl_head = T * (2 * H * H + 2 * H * V)
    vm = [r["enc_vocab_max"] for r in s]
    return {"what": "forward_sparse", "geometry": name, "hidden": H, "layers": L, "vocab": V, "m": M, "texts": len(lens),
            "tokens": T, "forward_ms": round(float(np.median(tf)), 4), "forward_ms_minmax": [round(min(tf), 4), round(max(tf), 4)],
            "forward_sparse_ms": round(float(np.median(ts)), 4), "forward_sparse_ms_minmax": [round(min(ts), 4), round(max(ts), 4)],
            "sparse_over_forward": round(float(np.median(ts) / np.median(tf)), 4),
            "flop_ratio": round((fl_fwd + fl_head) / fl_fwd, 4),
            "vocab_max_ms": round(med["enc_vocab_max"], 4), "vocab_max_ms_minmax": [round(min(vm), 4), round(max(vm), 4)],
            "vocab_max_tflops": round(2.0 * T * H * V / (med["enc_vocab_max"] * 1e-3) / 1e12, 2),
            "ffn1_ms_per_layer": round(med["enc_gemm_ffn1"] / L, 4),
            "ffn1_tflops": round(2.0 * T * H * F * L / (med["enc_gemm_ffn1"] * 1e-3) / 1e12, 2),
            "mlm_transform_ms": round(med["enc_mlm_rows"] + med["enc_mlm_dense"] + med["enc_mlm_ln"], 4),
            "topm_ms": round(med["enc_vocab_topm"], 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--full", action="store_true", help="also the full-size batch of 256 x 384 tokens")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "sparse.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.texts)
    lens = (224 + rng.integers(0, 64, size=a.texts)).tolist()
    geos = [("small-6", dict(BERT_SMALL_CFG, num_layers=6, pooling="cls")), ("base-12", dict(BERT_BASE_CFG, num_layers=12, pooling="cls"))]
    res = []
    for name, cfg in geos:
        res.append(run(name, cfg, lens, a.iters))
        print(json.dumps(res[-1]), flush=True)
        if a.full:
            res.append(run(name, dict(cfg, max_seq_len=384), [384] * 256, max(4, a.iters // 4)))
            print(json.dumps(res[-1]), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
