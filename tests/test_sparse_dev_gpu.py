"""GPU: the _dev forms of the sparse entry points (torch device pointers on torch's stream) against the host forms, with
and without dense_out / rows_out, across a growth of the encoder's buffers, in both compute modes."""
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder
from claude_semantic_search_amd.sparse_encoder import synth_mlm_head

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu

V, H, M = 1082, 384, 48


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_dev_forms_return_the_host_bits(mode):
    import torch

    cfg = br.BertCfg(num_layers=1, vocab=V, pooling="cls", **br.SMALL)
    enc = MpnetEncoder(synthetic_seed=3, compute=mode, cfg_overrides=cfg.encoder_overrides())
    enc.set_mlm_head(**synth_mlm_head(H, V, 3, bias_sigmas=-2.0))
    lib, st = nat.lib(), torch.cuda.current_stream().cuda_stream
    try:
        for lens in ([7, 33, 16, 1], [100, 64, 65, 17, 90, 120, 300]):      # (the second batch makes the buffers grow)
            batch = [[101] + np.random.default_rng(n).integers(1, V, size=n - 1).tolist() for n in lens]
            B, T = len(lens), sum(lens)
            terms, wts, nnz, z, rows = enc.encode_sparse_ids(batch, M, return_dense=True, return_rows=True)
            assert (nnz > 0).all()
            ids, cu = enc._pack_ids(batch)
            ids_d, cu_d = _dev(ids), _dev(cu)
            for with_dense, with_rows in ((True, True), (False, False), (True, False), (False, True)):
                t_d = torch.full((B, M), -9, dtype=torch.int32, device="cuda:0")
                w_d = torch.full((B, M), -9.0, dtype=torch.float32, device="cuda:0")
                n_d = torch.full((B,), -9, dtype=torch.int32, device="cuda:0")
                z_d = torch.full((B, V), -9.0, dtype=torch.float32, device="cuda:0") if with_dense else None
                r_d = torch.full((T, H), -9.0, dtype=torch.float32, device="cuda:0") if with_rows else None
                nat.check(lib.css_encoder_forward_sparse_dev(
                    enc._h, ids_d.data_ptr(), cu_d.data_ptr(), B, T, max(lens), M, t_d.data_ptr(), w_d.data_ptr(),
                    n_d.data_ptr(), z_d.data_ptr() if with_dense else None, r_d.data_ptr() if with_rows else None, st))
                torch.cuda.synchronize()
                assert np.array_equal(t_d.cpu().numpy(), terms) and np.array_equal(n_d.cpu().numpy(), nnz)
                assert np.array_equal(w_d.cpu().numpy().view(np.uint32), wts.view(np.uint32))
                if with_dense:
                    assert np.array_equal(z_d.cpu().numpy().view(np.uint32), z.view(np.uint32))
                if with_rows:
                    assert np.array_equal(r_d.cpu().numpy().view(np.uint32), rows.view(np.uint32))
            zz_d = torch.full((B, V), -9.0, dtype=torch.float32, device="cuda:0")
            nat.check(lib.css_encoder_vocab_max_dev(enc._h, _dev(rows).data_ptr(), cu_d.data_ptr(), B, T, zz_d.data_ptr(), st))
            torch.cuda.synchronize()
            assert np.array_equal(zz_d.cpu().numpy().view(np.uint32), z.view(np.uint32))
            assert np.array_equal(enc.vocab_max(rows, cu).view(np.uint32), z.view(np.uint32))
    finally:
        enc.close()
