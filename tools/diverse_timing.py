"""Device time of ``search_diverse(q, 10, fetch=128)`` next to ``search(q, 128)`` of the same build, on a synthetic
1 M x 768 index, for nq = 1 and nq = 1000: the difference is what the selection kernel (``k_mmr_select``) adds behind the
pool search.  Device-pointer calls between HIP events on one stream, warm-up first, the two calls interleaved, the
median of the repeats reported.  One JSON line per nq.  Development aid; not the benchmark.
usage: python tools/diverse_timing.py [rows] [reps]"""
import json
import statistics
import sys

sys.path.insert(0, ".")
import torch

from claude_semantic_search_amd import synth
from claude_semantic_search_amd.flat_index import IndexFlatIP

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
d, k, fetch, lam = 768, 10, 128, 0.5
stream = torch.cuda.current_stream()
st = stream.cuda_stream
ix = IndexFlatIP(d)
ix.reserve(rows)
ix.add_synthetic(rows, seed=7)
torch.cuda.synchronize()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


for nq in (1, 1000):
    q = torch.from_numpy(synth.rows(nq, d, 99)).cuda()
    Dp = torch.empty((nq, fetch), dtype=torch.float32, device="cuda")
    Ip = torch.empty((nq, fetch), dtype=torch.int64, device="cuda")
    Dk = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    Ik = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    plain = lambda: ix.search_dev(q.data_ptr(), nq, fetch, Dp.data_ptr(), Ip.data_ptr(), st, normalize=True)   # noqa: E731
    diverse = lambda: ix.search_diverse_dev(q.data_ptr(), nq, k, Dk.data_ptr(), Ik.data_ptr(), st, lam=lam, fetch=fetch,   # noqa: E731
                                            normalize=True)
    for _ in range(3):
        plain()
        diverse()
    torch.cuda.synchronize()
    tp, td = [], []
    for _ in range(reps):
        tp.append(timed(plain))
        td.append(timed(diverse))
    mp, md = statistics.median(tp), statistics.median(td)
    print(json.dumps({"rows": rows, "d": d, "nq": nq, "k": k, "fetch": fetch, "lam": lam, "reps": reps,
                      "search_128_ms": round(mp, 4), "search_diverse_ms": round(md, 4), "selection_ms": round(md - mp, 4),
                      "selection_read_bytes_per_query": (k - 1) * fetch * d * 4,
                      "search_128_ms_min_max": [round(min(tp), 4), round(max(tp), 4)],
                      "search_diverse_ms_min_max": [round(min(td), 4), round(max(td), 4)]}), flush=True)
ix.close()
