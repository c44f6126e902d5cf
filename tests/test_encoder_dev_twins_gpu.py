"""GPU: the two _dev twins that nothing else calls, css_encoder_forward_spans_dev and css_encoder_forward_pairs_dev
(device pointers on a caller's stream), return the bits of their host forms (encode_spans_ids, score_pair_ids) in both
compute modes.

Batches: [7, 33, 16, 1], then [100, 64, 65, 17, 90, 120], then 72 short sequences.  With the library's capacity
formulas the first batch leaves room for 512 tokens, 68 sequences, 80 spans and 70 pairs, which the second batch (456
tokens, 6 sequences, 18 spans) still fits; the third (612 tokens, 72 sequences, 216 spans) exceeds every one of them.
Its _dev call runs BEFORE the host call, so the activations grow inside the _dev form and the span / pair buffers
inside the host form."""
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.cross_encoder import synth_head
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = br.BertCfg(num_layers=1, vocab=1000, **br.SMALL)
BATCHES = ([7, 33, 16, 1], [100, 64, 65, 17, 90, 120], [3, 9, 17, 5] * 18)
H = 384


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module", params=["bf16", "fp32"])
def enc(request):
    e = MpnetEncoder(synthetic_seed=3, compute=request.param, cfg_overrides=CFG.encoder_overrides())
    h = synth_head(H, 3)
    e.set_head(h["pooler_w"], h["pooler_b"], h["cls_w"], h["cls_b"])
    yield e
    e.close()


def _spans(lens):
    """Per sequence a one-token span, the whole sequence and (from 3 tokens on) an interior span."""
    out = []
    for b, n in enumerate(lens):
        out += [(b, n // 2, n // 2 + 1), (b, 0, n)]
        if n >= 3:
            out.append((b, 1, n - 1))
    return np.asarray(out, dtype=np.int32)


def test_forward_spans_dev_returns_the_host_bits(enc):
    import torch

    lib, st = nat.lib(), torch.cuda.current_stream().cuda_stream
    query = np.random.default_rng(5).standard_normal(H).astype(np.float32)
    for lens in BATCHES:
        batch = br.synth_batch(CFG, lens, 4)
        B, T, spans = len(lens), sum(lens), _spans(lens)
        S = len(spans)
        ids, cu = enc._pack_ids(batch)
        ids_d, cu_d, sp_d, q_d = _dev(ids), _dev(cu), _dev(spans), _dev(query)
        got = {}
        for with_q in (False, True):
            for with_seq in (False, True):
                seq_d = torch.full((B, H), -7.0, dtype=torch.float32, device="cuda:0") if with_seq else None
                out_d = torch.full((S, H), -7.0, dtype=torch.float32, device="cuda:0")
                sc_d = torch.full((S,), -7.0, dtype=torch.float32, device="cuda:0") if with_q else None
                nat.check(lib.css_encoder_forward_spans_dev(
                    enc._h, ids_d.data_ptr(), cu_d.data_ptr(), B, T, max(lens), sp_d.data_ptr(), S,
                    q_d.data_ptr() if with_q else None, 1, seq_d.data_ptr() if with_seq else None, out_d.data_ptr(),
                    sc_d.data_ptr() if with_q else None, st))
                torch.cuda.synchronize()
                got[with_q, with_seq] = (seq_d, out_d, sc_d)
        for with_q in (False, True):
            seq, out, scores = enc.encode_spans_ids(batch, spans, normalize=True, query=query if with_q else None)
            for with_seq in (False, True):
                seq_d, out_d, sc_d = got[with_q, with_seq]
                assert np.array_equal(_bits(out_d), out.view(np.uint32)), (lens, with_q, with_seq)
                if with_seq:
                    assert np.array_equal(_bits(seq_d), seq.view(np.uint32)), (lens, with_q)
                if with_q:
                    assert np.array_equal(_bits(sc_d), scores.view(np.uint32)), (lens, with_seq)
    # scores alone (no span rows), and the argument rule the twin shares with the host form
    sc_d = torch.full((S,), -7.0, dtype=torch.float32, device="cuda:0")
    nat.check(lib.css_encoder_forward_spans_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), B, T, max(lens), sp_d.data_ptr(), S,
                                                q_d.data_ptr(), 1, None, None, sc_d.data_ptr(), st))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sc_d), scores.view(np.uint32))
    assert lib.css_encoder_forward_spans_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), B, T, max(lens), sp_d.data_ptr(), S,
                                             q_d.data_ptr(), 1, None, None, None, st) != 0
    assert "css_encoder_forward_spans_dev: q and scores_out go together" in nat.last_error()


def test_forward_pairs_dev_returns_the_host_bits(enc):
    import torch

    lib, st = nat.lib(), torch.cuda.current_stream().cuda_stream
    for lens in BATCHES:
        batch = br.synth_batch(CFG, lens, 6)
        B, T = len(lens), sum(lens)
        seg = np.asarray([max(1, n // 2) for n in lens], dtype=np.int32)
        ids, cu = enc._pack_ids(batch)
        ids_d, cu_d, seg_d = _dev(ids), _dev(cu), _dev(seg)
        lg_d = torch.full((B,), -7.0, dtype=torch.float32, device="cuda:0")
        nat.check(lib.css_encoder_forward_pairs_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), seg_d.data_ptr(), B, T, max(lens),
                                                    lg_d.data_ptr(), st))
        torch.cuda.synchronize()
        want = enc.score_pair_ids(batch, seg)
        assert np.isfinite(want).all() and len(set(want.tolist())) > 1
        assert np.array_equal(_bits(lg_d), want.view(np.uint32)), lens


def test_forward_pairs_dev_names_itself_without_a_head():
    import torch

    e = MpnetEncoder(synthetic_seed=3, cfg_overrides=CFG.encoder_overrides())
    try:
        t = _dev(np.asarray([0, 3], dtype=np.int32))
        assert nat.lib().css_encoder_forward_pairs_dev(e._h, t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 3, 3, t.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream) != 0
        assert "css_encoder_forward_pairs_dev: no classification head" in nat.last_error()
    finally:
        e.close()
