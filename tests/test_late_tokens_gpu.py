"""GPU: css_encoder_forward_tokens against the device's own fp32 token rows (debug_read("x32")), and the neutrality
of the late-interaction calls towards the encoder's other entry points."""
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.late_interaction import bf16_to_f32, synth_projection
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu

GEOS = {"small": br.SMALL, "base": br.BASE}
LENS = [1, 16, 17, 33, 100, 7]          # 174 tokens: the last block of 16 is partial, sequences straddle the blocks
WSEED, BSEED = 11, 5


def _cfg(geo, pooling="mean"):
    return br.BertCfg(num_layers=2, vocab=2000, pooling=pooling, **GEOS[geo])


def _bf16_ulp(x):
    """One unit in the last place of the bf16 numbers of x's magnitude (8 significant bits)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 7)


# ---- 3. token vectors against the device's own rows ---------------------------------------------------------------------
@pytest.mark.parametrize("P", [None, 96, 128])
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_token_vectors_are_the_projected_rows(geo, compute, P):
    """tok_out is within one bf16 unit in the last place of normalize(W x_t) formed in float64 from the fp32 rows the
    forward left in x32: half a unit is the one rounding, the rest the fp32 accumulation of the projection, which is a
    larger share of the last place of a component near zero (measured: 0.500 without a projection, up to 0.976 with
    one); seq_out is what encode_ids returns, bit for bit."""
    cfg = _cfg(geo)
    T, H = sum(LENS), cfg.hidden
    assert T < 1024 and T % 16
    batch = br.synth_batch(cfg, LENS, BSEED)
    enc = MpnetEncoder(synthetic_seed=WSEED, compute=compute, cfg_overrides=cfg.encoder_overrides())
    W = None
    if P is not None:
        W = synth_projection(H, P, WSEED)
        enc.set_token_projection(W)
    assert enc.token_dim == (P or H)
    want_seq = enc.encode_ids(batch)
    for normalize in (True, False):
        mats, seq = enc.encode_tokens_ids(batch, normalize=normalize, return_seq=True)
        x = enc.debug_read("x32", (T, H)).astype(np.float64)
        assert [m.shape for m in mats] == [(n, P or H) for n in LENS] and all(m.dtype == np.uint16 for m in mats)
        v = x @ W.astype(np.float64).T if W is not None else x
        if normalize:
            v = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
        got = bf16_to_f32(np.concatenate(mats)).astype(np.float64)
        ulps = float((np.abs(got - v) / _bf16_ulp(v)).max())
        print(f"[late tokens] {geo} {compute} P={P} normalize={normalize}: max error = {ulps:.3f} bf16 ulp")
        assert ulps <= 1.0
        if normalize:
            assert np.array_equal(seq.view(np.uint32), want_seq.view(np.uint32))
            again = enc.encode_tokens_ids(batch, normalize=True)
            assert all(np.array_equal(a, b) for a, b in zip(mats, again))
    enc.close()


# ---- 6. neutrality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [[12], [128, 6, 64, 33, 255], [300, 280, 260, 200]], ids=["graph", "unfolded", "folded"])
@pytest.mark.parametrize("geo", ["small", "base"])
def test_other_entry_points_keep_their_bits(geo, lens):
    """encode_ids (one 12-token sequence: eager, captured, replayed), encode_spans_ids and score_pair_ids return the
    same bits before and after late-interaction calls on the same encoder, with and without a projection."""
    cfg = _cfg(geo, pooling="cls")
    batch = br.synth_batch(cfg, lens, BSEED)
    spans = [(b, 0, n) for b, n in enumerate(lens)] + [(0, 1, min(lens[0], 9))]
    seg = [max(1, n // 2) for n in lens]
    enc = MpnetEncoder(synthetic_seed=WSEED, compute="bf16", cfg_overrides=cfg.encoder_overrides())
    H = cfg.hidden
    rng = np.random.default_rng(1)
    enc.set_head(rng.standard_normal((H, H)).astype(np.float32) * 0.02, np.zeros(H, np.float32),
                 rng.standard_normal(H).astype(np.float32) * 0.05, np.zeros(1, np.float32))

    def snapshot():
        a = enc.encode_ids(batch)
        b = enc.encode_ids(batch)
        s = enc.encode_spans_ids(batch, spans)
        return a, b, s[0], s[1], enc.score_pair_ids(batch, seg)

    before = snapshot()
    mats = enc.encode_tokens_ids(batch)
    enc.maxsim([mats[0][:8]], mats)
    enc.score_late_ids(batch, [mats[0][:8]])
    enc.set_token_projection(synth_projection(H, 96, WSEED))
    q = enc.encode_tokens_ids(batch)[0][:8]
    enc.score_late_ids(batch, [q])
    mid = snapshot()
    enc.set_token_projection(None)
    after = snapshot()
    for x, y, z in zip(before, mid, after):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
    enc.close()
