"""GPU: the _dev forms of the late-interaction entry points (device pointers on a caller's stream) against the host
forms, and what only they do: indices clamped into range, a query's tokens beyond 64 ignored, a doc with no kept token
scoring 0, the encoder's own token buffer when tok_out is NULL."""
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.late_interaction import synth_projection
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import late_cases as lt  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    return t.to("cuda:0")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def enc():
    cfg = br.BertCfg(num_layers=1, vocab=1000, **br.SMALL)
    e = MpnetEncoder(synthetic_seed=3, cfg_overrides=cfg.encoder_overrides())
    e.set_token_projection(synth_projection(384, 96, 3))
    yield e
    e.close()


def test_forward_tokens_dev_and_forward_maxsim_dev_return_the_host_bits(enc):
    import torch

    lib, st = nat.lib(), torch.cuda.current_stream().cuda_stream
    cfg = br.BertCfg(num_layers=1, vocab=1000, **br.SMALL)
    P = enc.token_dim
    for lens in ([7, 33, 16, 1], [100, 64, 65, 17, 90, 120]):           # (the second batch makes the token buffer grow)
        batch = br.synth_batch(cfg, lens, 4)
        B, T = len(lens), sum(lens)
        mats, seq = enc.encode_tokens_ids(batch, return_seq=True)
        q = [mats[1][:9], mats[0][:5]]
        keep = [np.ones(n, np.uint8) for n in lens]
        keep[1][::2] = 0
        pairs = [(0, j) for j in range(B)] + [(1, 0)]
        want = enc.score_late_ids(batch, q, pairs=pairs, keep=keep)
        ids, cu = enc._pack_ids(batch)
        ids_d, cu_d = _dev(ids), _dev(cu)
        tok_d = torch.empty((T, P), dtype=torch.int16, device="cuda:0")
        seq_d = torch.empty((B, 384), dtype=torch.float32, device="cuda:0")
        nat.check(lib.css_encoder_forward_tokens_dev(enc._h, ids_d.data_ptr(), cu_d.data_ptr(), B, T, max(lens), 1,
                                                     tok_d.data_ptr(), seq_d.data_ptr(), st))
        torch.cuda.synchronize()
        assert np.array_equal(_host(tok_d, np.uint16), np.concatenate(mats))
        assert np.array_equal(_host(seq_d, np.uint32), seq.view(np.uint32))
        qr, cuq, _ = enc._pack_mats("q", q)
        q_d, cuq_d, keep_d = _dev(qr), _dev(cuq), _dev(np.concatenate(keep))
        pr_d = _dev(np.asarray(pairs, np.int32))
        for tok_out in (None, torch.zeros((T, P), dtype=torch.int16, device="cuda:0")):
            sc_d = torch.full((len(pairs),), -7.0, dtype=torch.float32, device="cuda:0")
            nat.check(lib.css_encoder_forward_maxsim_dev(
                enc._h, ids_d.data_ptr(), cu_d.data_ptr(), B, T, max(lens), q_d.data_ptr(), cuq_d.data_ptr(), len(q),
                keep_d.data_ptr(), pr_d.data_ptr(), len(pairs), sc_d.data_ptr(),
                tok_out.data_ptr() if tok_out is not None else None, st))
            torch.cuda.synchronize()
            assert np.array_equal(_host(sc_d, np.uint32), want.view(np.uint32))
            if tok_out is not None:
                assert np.array_equal(_host(tok_out, np.uint16), np.concatenate(mats))


@pytest.mark.parametrize("P", [64, 128])
def test_maxsim_dev_clamps_where_the_host_form_refuses(enc, P):
    import torch

    lib, st = nat.lib(), torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(P)
    q = [lt.to_bf16(rng.integers(-1, 2, size=(m, P)).astype(np.float32)) for m in (70, 3)]     # 70 > 64 tokens
    d = [lt.to_bf16(rng.integers(-1, 2, size=(m, P)).astype(np.float32)) for m in (20, 33, 5)]
    keep = [np.ones(20, np.uint8), np.zeros(33, np.uint8), np.ones(5, np.uint8)]            # doc 1: nothing kept
    keep[0][3] = 0
    pairs = [(0, 0), (1, 1), (-3, 99), (7, -1), (1, 2), (0, 1)]
    with pytest.raises(RuntimeError, match="query 0 has 70 tokens"):
        enc.maxsim(q, d)
    # what the clamps mean, through the host form: the first 64 query tokens, indices moved to the nearest valid one
    host = enc.maxsim([q[0][:64], q[1]], [d[0], d[2]], pairs=[(0, 0), (0, 1), (1, 0), (1, 1)], keep=[keep[0], keep[2]])
    want = np.array([host[0], 0.0, host[1], host[2], host[3], 0.0], dtype=np.float32)
    qr, cuq, _ = enc._pack_mats("q", q)
    dr, cud, _ = enc._pack_mats("d", d)
    t = [_dev(x) for x in (qr, cuq, dr, cud, np.concatenate(keep), np.asarray(pairs, np.int32))]
    sc_d = torch.full((len(pairs),), -7.0, dtype=torch.float32, device="cuda:0")
    for _ in range(2):
        nat.check(lib.css_encoder_maxsim_dev(enc._h, t[0].data_ptr(), t[1].data_ptr(), 2, t[2].data_ptr(), t[3].data_ptr(), 3,
                                             t[4].data_ptr(), t[5].data_ptr(), len(pairs), P, sc_d.data_ptr(), st))
        torch.cuda.synchronize()
        assert np.array_equal(_host(sc_d, np.uint32), want.view(np.uint32)), (_host(sc_d, np.float32), want)
    assert lib.css_encoder_maxsim_dev(enc._h, t[0].data_ptr(), t[1].data_ptr(), 2, t[2].data_ptr(), t[3].data_ptr(), 3,
                                      None, t[5].data_ptr(), len(pairs), 48, sc_d.data_ptr(), st) != 0
    assert "P=48" in nat.last_error()
