"""GPU: css_encoder_forward_sparse on 2-layer models (both geometries, both compute modes) against the device's own
rows, float64 log1p, the PyTorch fp32 reference, and the neutrality of the sparse calls towards the encoder's other
entry points."""
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.late_interaction import synth_projection
from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder
from claude_semantic_search_amd.sparse_encoder import synth_mlm_head

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import splade_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

M = sr.M
GEOS = ["small", "base"]
MODES = ["fp32", "bf16"]


def _cfg(geo):
    return br.BertCfg(num_layers=2, pooling="cls", normalize=False, **sr.GEOS[geo])


@lru_cache(maxsize=None)
def weights(geo):
    return sr.synth_weights(_cfg(geo), sr.WSEEDS[geo])


@lru_cache(maxsize=None)
def reference(geo, length, index):
    """The reference's result for sequence `index` of a batch (synth_batch seeds a sequence by its position)."""
    cfg = _cfg(geo)
    ids = br.synth_batch(cfg, [1] * index + [length], sr.BSEED)[index]
    return sr.sparse(weights(geo), cfg, ids)


def make_encoder(geo, mode):
    cfg = _cfg(geo)
    enc = MpnetEncoder(synthetic_seed=sr.WSEEDS[geo], compute=mode, cfg_overrides=cfg.encoder_overrides())
    enc.set_mlm_head(**synth_mlm_head(cfg.hidden, cfg.vocab, sr.WSEEDS[geo]))
    return enc


def run(enc, geo, lens):
    batch = br.synth_batch(_cfg(geo), lens, sr.BSEED)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return batch, cu, enc.encode_sparse_ids(batch, M, return_dense=True, return_rows=True)


def z_errors(enc, geo, cases):
    """Largest |z - z_ref| over the batches, and the results."""
    worst, outs = 0.0, []
    for lens in cases:
        _, _, out = run(enc, geo, lens)
        for b, n in enumerate(lens):
            worst = max(worst, float(np.abs(out[3][b] - reference(geo, n, b)["z"]).max()))
        outs.append(out)
    return worst, outs


# ---- 1-3. the call against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geo", GEOS)
def test_dense_rows_and_weights_agree(geo, mode):
    """dense_out is vocab_max(rows_out) bit for bit; rows_out is g formed in float64 from the device's own x32 within
    the bar of one fp32 GEMM of depth H plus the LayerNorm (unfolded path); the lists are the exact top-m of dense_out
    and weights_out is within one fp32 unit in the last place of float64 log1p; the same call gives the same bits."""
    enc = make_encoder(geo, mode)
    cfg, w = _cfg(geo), weights(geo)
    try:
        for lens in sr.CASES + [sr.BIG_CASE]:
            batch, cu, (terms, wts, nnz, z, rows) = run(enc, geo, lens)
            T = int(cu[-1])
            folded = geo == "base" and mode == "bf16" and T >= 1024
            if not folded:
                x = enc.debug_read("x32", (T, cfg.hidden))
                g64 = sr.rows64(w, cfg, x)
                umin = min(reference(geo, n, b)["umin"] for b, n in enumerate(lens))
                bar = sr.fp32_rows_bar(w, cfg, x, umin)
                err = float(np.abs(rows - g64).max())
                print(f"[sparse rows] {geo} {mode} {lens}: max |g - g64| = {err:.3e}, bar {bar:.3e}")
                assert err <= bar
            assert np.array_equal(enc.vocab_max(rows, cu).view(np.uint32), z.view(np.uint32))
            assert (z >= 0).all()
            for b in range(len(lens)):
                t_ref, w_ref, n_ref = sr.topm(z[b], M)
                assert nnz[b] == n_ref and np.array_equal(terms[b], t_ref)
                assert np.all(np.abs(wts[b].view(np.int32) - w_ref.view(np.int32)) <= 1)
            again = enc.encode_sparse_ids(batch, M, return_dense=True)
            assert all(np.array_equal(a, b) for a, b in zip((terms, wts, nnz, z), again))
    finally:
        enc.close()


# ---- 4. fp32 mode against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_fp32_against_the_reference(geo):
    """|w - w_ref| <= |z - z_ref| <= the bar propagated from the project's 1e-4 per hidden component
    (splade_reference.fp32_z_bar; DESIGN.md 3.3e has the values)."""
    enc = make_encoder(geo, "fp32")
    cfg, w = _cfg(geo), weights(geo)
    try:
        for lens in sr.CASES + [sr.BIG_CASE]:
            _, _, (terms, wts, nnz, z, rows) = run(enc, geo, lens)
            for b, n in enumerate(lens):
                ref = reference(geo, n, b)
                bar = sr.fp32_z_bar(w, cfg, ref["umin"])
                dz = float(np.abs(z[b] - ref["z"]).max())
                k = min(M, int(nnz[b]))
                dw = float(np.abs(wts[b, :k] - ref["w"][terms[b, :k]]).max()) if k else 0.0
                print(f"[sparse fp32] {geo} len {n}: |z - z_ref| = {dz:.3e}, |w - w_ref| = {dw:.3e}, bar {bar:.3e}, nnz {nnz[b]}")
                assert dz <= bar and dw <= bar
                check_lists(terms[b], nnz[b], ref, bar)
    finally:
        enc.close()


def check_lists(terms, nnz, ref, bar):
    """Lists against the reference where it can tell: every reference term more than 2 bar above the reference's cut
    weight is returned, and nnz lies between the counts of reference logits above +bar and above -bar."""
    lm = ref["logit_max"]
    assert int((lm > bar).sum()) <= int(nnz) <= int((lm > -bar).sum())
    order = np.argsort(-ref["z"], kind="stable")
    cut = ref["z"][order[M]] if int((ref["z"] > 0).sum()) > M else 0.0
    must = order[:M][ref["z"][order[:M]] > cut + 2 * bar]
    assert np.isin(must, terms).all()


# ---- 5, 6. bf16 mode against the fp32 reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_bf16_against_the_reference(geo):
    """The bar on |z - z_ref| is twice the largest figure measured over these batches (splade_reference.BF16_Z_MEASURED);
    the big batch takes the LayerNorm-folded path at hidden 768 and is repeated with the running-maximum softmax
    (set_attention_range(0))."""
    enc = make_encoder(geo, "bf16")
    bar = 2 * sr.BF16_Z_MEASURED["2layer"]
    try:
        worst, outs = z_errors(enc, geo, sr.CASES + [sr.BIG_CASE])
        enc.set_attention_range(0)
        worst0, outs0 = z_errors(enc, geo, [sr.BIG_CASE])
        print(f"[sparse bf16] {geo}: max |z - z_ref| = {worst:.3e} (attention range 0, big batch: {worst0:.3e}), bar {bar:.3e}")
        assert worst <= bar and worst0 <= bar
        for lens, out in zip(sr.CASES + [sr.BIG_CASE, sr.BIG_CASE], outs + outs0):
            for b, n in enumerate(lens):
                check_lists(out[0][b], out[2][b], reference(geo, n, b), bar)
    finally:
        enc.close()


# ---- 7. neutrality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [[12], [128, 6, 64, 33, 255], [300, 280, 260, 200]], ids=["graph", "unfolded", "folded"])
@pytest.mark.parametrize("geo", GEOS)
def test_other_entry_points_keep_their_bits(geo, lens):
    """encode_ids (one 12-token sequence: eager, captured, replayed), encode_spans_ids, score_pair_ids, encode_tokens_ids
    and maxsim return the same bits before and after sparse calls and before and after set_mlm_head."""
    cfg = br.BertCfg(num_layers=2, vocab=2000, pooling="cls", **sr.GEOS[geo])
    batch = br.synth_batch(cfg, lens, sr.BSEED)
    spans = [(b, 0, n) for b, n in enumerate(lens)] + [(0, 1, min(lens[0], 9))]
    seg = [max(1, n // 2) for n in lens]
    enc = MpnetEncoder(synthetic_seed=11, compute="bf16", cfg_overrides=cfg.encoder_overrides())
    H = cfg.hidden
    rng = np.random.default_rng(1)
    enc.set_head(rng.standard_normal((H, H)).astype(np.float32) * 0.02, np.zeros(H, np.float32),
                 rng.standard_normal(H).astype(np.float32) * 0.05, np.zeros(1, np.float32))
    enc.set_token_projection(synth_projection(H, 96, 11))

    def snapshot():
        a = enc.encode_ids(batch)
        b = enc.encode_ids(batch)
        c = enc.encode_ids(batch)
        s = enc.encode_spans_ids(batch, spans)
        mats = enc.encode_tokens_ids(batch)
        return a, b, c, s[0], s[1], enc.score_pair_ids(batch, seg), np.concatenate(mats), enc.maxsim([mats[0][:8]], mats)

    try:
        before = snapshot()
        head = synth_mlm_head(H, cfg.vocab, 11, bias_sigmas=-2.0)
        enc.set_mlm_head(**head)
        mid = snapshot()
        out = enc.encode_sparse_ids(batch, 64, return_dense=True, return_rows=True)
        enc.vocab_max(out[4], np.concatenate([[0], np.cumsum(lens)]))
        after = snapshot()
        enc.set_mlm_head(**dict(head, decoder_w=rng.standard_normal((cfg.vocab, H)).astype(np.float32) * 0.02))
        enc.encode_sparse_ids(batch, 512)
        last = snapshot()
        for x, *rest in zip(before, mid, after, last):
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for y in rest)
    finally:
        enc.close()


def test_errors_name_the_argument():
    from claude_semantic_search_amd import _native as nat

    cfg = br.BertCfg(num_layers=1, vocab=500, pooling="cls", **br.SMALL)
    enc = MpnetEncoder(synthetic_seed=3, compute="bf16", cfg_overrides=cfg.encoder_overrides())
    batch = [[101, 7, 102], [101, 102]]
    try:
        with pytest.raises(RuntimeError, match="no masked-LM head"):
            enc.encode_sparse_ids(batch, 8)
        with pytest.raises(RuntimeError, match="no masked-LM head"):
            enc.vocab_max(np.zeros((3, 384), np.float32), [0, 3])
        enc.set_mlm_head(**synth_mlm_head(384, 500, 3))
        for m in (0, 513):
            with pytest.raises(RuntimeError, match=f"m={m}"):
                enc.encode_sparse_ids(batch, m)
        with pytest.raises(RuntimeError, match="sequence 1 has length 0"):
            enc.vocab_max(np.zeros((3, 384), np.float32), [0, 3, 3])
        with pytest.raises(RuntimeError, match="token 1 has id 500"):
            enc.encode_sparse_ids([[101, 500, 102]], 8)
        terms, _, nnz = enc.encode_sparse_ids(batch, 8)          # the refused calls left the head in place
        assert terms.shape == (2, 8) and (nnz >= 0).all()
    finally:
        enc.close()
    mp = MpnetEncoder(synthetic_seed=3, compute="bf16", cfg_overrides={"num_layers": 1})
    try:
        z = np.zeros(768, np.float32)
        rc = nat.lib().css_encoder_set_mlm_head(mp._h, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, None,
                                                z.ctypes.data)
        assert rc == -1 and b"BERT" in nat.lib().css_last_error()
    finally:
        mp.close()
