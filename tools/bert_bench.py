"""Encoder throughput of MPNet (12 layers) next to the all-MiniLM-L6-v2 geometry (BERT, 6 x hidden 384 / ffn 1536),
synthetic weights, one process, bf16 product mode.

    python tools/bert_bench.py [--batch 256] [--seq 384] [--iters 10] [--models mpnet,minilm] [--json out.json]

For each model: ms per batch of `batch` chunks of `seq` tokens (HIP events around css_encoder_forward_dev on the
current stream, after warm-up), chunks/s, the fraction of the 2500 TFLOP/s dense bf16 peak, and the single-query
latency (one 24-token chunk through css_encoder_forward, host wall clock, median after the graph is captured).
FLOPs per sequence of L tokens: layers * (2 L (4 H^2 + 2 H F) + 4 L^2 H).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from claude_semantic_search_amd import _native as nat  # noqa: E402
from claude_semantic_search_amd.mpnet_encoder import BERT_SMALL_CFG, MpnetEncoder  # noqa: E402

PEAK_TFLOPS = 2500.0
MODELS = {"mpnet": {}, "minilm": dict(BERT_SMALL_CFG)}


def flops(cfg: dict, lengths) -> float:
    H, F, nl = cfg["hidden"], cfg["ffn"], cfg["num_layers"]
    return float(sum(nl * (2 * L * (4 * H * H + 2 * H * F) + 4 * L * L * H) for L in lengths))


def run(name: str, batch: int, seq: int, iters: int) -> dict:
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides=MODELS[name] or None)
    cfg = enc.cfg
    rng = np.random.default_rng(0)
    ids = rng.integers(1000, cfg["vocab"], size=batch * seq, dtype=np.int32)
    cu = np.arange(batch + 1, dtype=np.int32) * seq
    dev = torch.device("cuda:0")
    ids_d, cu_d = torch.from_numpy(ids).to(dev), torch.from_numpy(cu).to(dev)
    out_d = torch.empty((batch, cfg["hidden"]), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream()

    def fwd():
        nat.check(nat.lib().css_encoder_forward_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), batch, batch * seq, seq,
                                                    1, out_d.data_ptr(), stream.cuda_stream))

    for _ in range(3):
        fwd()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fwd()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    ms = statistics.median(times)
    fl = flops(cfg, [seq] * batch)
    q = [rng.integers(1000, cfg["vocab"], size=24).tolist()]
    for _ in range(5):
        enc.encode_ids(q)
    lat = []
    for _ in range(50):
        t0 = time.perf_counter()
        enc.encode_ids(q)
        lat.append((time.perf_counter() - t0) * 1e3)
    enc.close()
    return {"model": name, "layers": cfg["num_layers"], "hidden": cfg["hidden"], "ffn": cfg["ffn"],
            "batch": batch, "seq": seq, "ms_per_batch": round(ms, 3), "ms_min": round(min(times), 3),
            "chunks_per_s": round(batch / ms * 1e3, 1), "tflop_per_batch": round(fl / 1e12, 3),
            "frac_bf16_peak": round(fl / (ms * 1e-3) / 1e12 / PEAK_TFLOPS, 4),
            "single_query_ms": round(statistics.median(lat), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=384)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--models", default="mpnet,minilm")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = [run(m, a.batch, a.seq, a.iters) for m in a.models.split(",")]
    for r in res:
        print(json.dumps(r))
    names = [r["model"] for r in res]
    if "mpnet" in names and "minilm" in names:
        mp, ml = res[names.index("mpnet")], res[names.index("minilm")]
        print(json.dumps({"minilm_over_mpnet_time": round(ml["ms_per_batch"] / mp["ms_per_batch"], 4)}))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
