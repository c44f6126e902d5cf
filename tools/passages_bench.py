"""What span pooling costs: css_encoder_forward_spans against css_encoder_forward of the same batch, and against encoding
every passage as a text of its own.  Synthetic weights, 12 layers, bf16 product mode, one process.

    python tools/passages_bench.py [--texts 2,10,256] [--seq 384] [--passages 20] [--iters 20] [--json profiles/passages.json]

Per shape (`texts` sequences of `seq` tokens, `passages` spans each that tile tokens 1..seq-2; 10 texts = the top-10 of
a search, 256 texts = an indexing batch -- both hold >= 1024 tokens and take the LayerNorm-folded path with
k_span_pool_ln; 2 texts = 768 tokens stay on the unfolded bf16 path with k_span_pool):
  * device time (HIP events on the stream, `forward_dev` and `forward_spans_dev` alternating, median and min of `iters`);
  * the span kernel alone (the library's own event pair around its launch, css_prof_read("enc_span_pool"));
  * host wall clock of `encode_ids`, `encode_spans_ids` (rows + scores) and of `encode_ids` over every passage as a
    sequence of its own (`<s>` passage `</s>`, 256 passages per call): what the span pooling replaces.
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
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder  # noqa: E402


def wall(fn, iters: int):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def run(enc: MpnetEncoder, texts: int, seq: int, passages: int, iters: int) -> dict:
    H = enc.cfg["hidden"]
    rng = np.random.default_rng(texts)
    ids = rng.integers(1000, enc.cfg["vocab"], size=(texts, seq), dtype=np.int32)
    ids[:, 0], ids[:, -1] = 0, 2
    cuts = np.linspace(1, seq - 1, passages + 1).round().astype(np.int32)
    spans = np.array([(b, cuts[i], cuts[i + 1]) for b in range(texts) for i in range(passages)], dtype=np.int32)
    S = len(spans)
    q = rng.standard_normal(H).astype(np.float32)
    q /= np.linalg.norm(q)
    dev = torch.device("cuda:0")
    ids_d = torch.from_numpy(ids.reshape(-1)).to(dev)
    cu_d = torch.from_numpy(np.arange(texts + 1, dtype=np.int32) * seq).to(dev)
    sp_d, q_d = torch.from_numpy(spans.reshape(-1)).to(dev), torch.from_numpy(q).to(dev)
    seq_d = torch.empty((texts, H), dtype=torch.float32, device=dev)
    out_d = torch.empty((S, H), dtype=torch.float32, device=dev)
    sc_d = torch.empty(S, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream()
    lib = nat.lib()

    def fwd():
        nat.check(lib.css_encoder_forward_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), texts, texts * seq, seq, 1,
                                              seq_d.data_ptr(), stream.cuda_stream))

    def fwd_spans():
        nat.check(lib.css_encoder_forward_spans_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), texts, texts * seq, seq,
                                                    sp_d.data_ptr(), S, q_d.data_ptr(), 1, seq_d.data_ptr(),
                                                    out_d.data_ptr(), sc_d.data_ptr(), stream.cuda_stream))

    def timed(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        fwd()
        fwd_spans()
    torch.cuda.synchronize()
    t_f, t_s = [], []
    for _ in range(iters):          # alternating: both see the same clocks and the same neighbours
        t_f.append(timed(fwd))
        t_s.append(timed(fwd_spans))
    nat.prof_reset()
    nat.prof_enable(True)
    for _ in range(iters):
        fwd_spans()
    torch.cuda.synchronize()
    k_ms, k_n = nat.prof_read("enc_span_pool")
    nat.prof_enable(False)
    batch = [row.tolist() for row in ids]
    own = [[0] + ids[b, lo:hi].tolist() + [2] for b, lo, hi in spans]
    host_iters = max(3, iters // 4)
    w_f = wall(lambda: enc.encode_ids(batch), host_iters)
    w_s = wall(lambda: enc.encode_spans_ids(batch, spans, query=q), host_iters)
    w_o = wall(lambda: [enc.encode_ids(own[i:i + 256]) for i in range(0, S, 256)], host_iters)
    med_f, med_s = statistics.median(t_f), statistics.median(t_s)
    return {"texts": texts, "seq": seq, "spans": S, "tokens": texts * seq, "folded_path": texts * seq >= 1024,
            "forward_ms": round(med_f, 4), "forward_ms_min": round(min(t_f), 4),
            "forward_spans_ms": round(med_s, 4), "forward_spans_ms_min": round(min(t_s), 4),
            "spans_over_forward": round(med_s / med_f, 4), "span_kernel_ms": round(k_ms / max(k_n, 1), 4),
            "span_rows_read_mb": round(float((spans[:, 2] - spans[:, 1]).sum()) * H * (2 if texts * seq >= 1024 else 4) / 1e6, 2),
            "host_encode_ids_ms": round(w_f[0], 3), "host_encode_spans_ids_ms": round(w_s[0], 3),
            "host_every_passage_alone_ms": round(w_o[0], 3),
            "alone_over_spans": round(w_o[0] / w_s[0], 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", default="2,10,256")
    ap.add_argument("--seq", type=int, default=384)
    ap.add_argument("--passages", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "passages.json"))
    a = ap.parse_args()
    enc = MpnetEncoder(synthetic_seed=1, compute="bf16", cfg_overrides={"num_layers": a.layers})
    res = [run(enc, int(t), a.seq, a.passages, a.iters) for t in a.texts.split(",")]
    enc.close()
    for r in res:
        print(json.dumps(r), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
