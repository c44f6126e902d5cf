"""Vocabulary maximum and top-m on lattice inputs, bit for bit (css_encoder_vocab_max, css_encoder_forward_sparse).

Rows and decoder E have components in {-1, 0, 1} or {-8..8}/8 and the bias c holds multiples of 1/64: every product and
every partial sum is then a multiple of 1/64 below 2^24 / 64, exact in bf16 operands and fp32 accumulation whatever the
order, so zmax must equal the float64 truth bit for bit in both compute modes."""
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder
from claude_semantic_search_amd.sparse_encoder import synth_mlm_head

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bert_reference as br  # noqa: E402
import splade_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

VOCABS = [1, 58, 256, 314, 1082]
LENGTH_SETS = [[1], [1] * 40, [15, 16, 17], [255, 256, 257], [3, 250, 3, 300], [512, 512, 5]]


def short_seqs():
    """200 sequences of 1-3 tokens."""
    return (1 + np.random.default_rng(5).integers(0, 3, size=200)).tolist()


def lattice(rng, shape, kind):
    if kind == "unit":
        return rng.integers(-1, 2, size=shape).astype(np.float32)
    return (rng.integers(-8, 9, size=shape) / 8.0).astype(np.float32)


def make_encoder(hidden, mode, vocab):
    geo = br.SMALL if hidden == 384 else br.BASE
    cfg = br.BertCfg(num_layers=1, pooling="cls", normalize=False, vocab=vocab, **geo)
    return MpnetEncoder(synthetic_seed=3, compute=mode, cfg_overrides=cfg.encoder_overrides())


def set_lattice_head(enc, E, c):
    H, V = E.shape[1], E.shape[0]
    h = synth_mlm_head(H, V, 3)
    enc.set_mlm_head(h["dense_w"], h["dense_b"], h["ln_g"], h["ln_b"], E, c)


def truth(rows, cu, E, c):
    """relu(max_t (rows E^T + c)) per sequence in float64, as float32 (exact on the lattice)."""
    logits = rows.astype(np.float64) @ E.astype(np.float64).T + c.astype(np.float64)
    z = np.stack([logits[cu[b]:cu[b + 1]].max(axis=0) for b in range(len(cu) - 1)])
    return np.maximum(z, 0.0).astype(np.float32)


def planted_case(rng, lens, E, c, kind):
    """Lattice rows for the length set with, per sequence, one token equal to a row of E (a logit far above the rest):
    in the first token, the last, the last row of a 256-row tile and the first row of the next where the sequence has
    them, neighbouring sequences taking different terms; the third sequence of a set (when there is one) is all zero
    rows, so with c < 0 every one of its logits is negative."""
    V, H = E.shape
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = lattice(rng, (int(cu[-1]), H), kind)
    for b, L in enumerate(lens):
        lo, hi = int(cu[b]), int(cu[b + 1])
        spots = [lo, hi - 1] + [t for t in (255, 256, 511, 512, 767, 768) if lo <= t < hi]
        for j, t in enumerate(spots):
            rows[t] = E[(7 * b + 3 * j + 1) % V]
        if b == 2 and len(lens) > 2:
            rows[lo:hi] = 0.0
    return rows, cu


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("hidden", [384, 768])
def test_vocab_max_lattice_exact(hidden, mode):
    rng = np.random.default_rng(hidden + (mode == "bf16"))
    for V in VOCABS:
        enc = make_encoder(hidden, mode, V)
        try:
            for kind in ("unit", "eighths"):
                E = lattice(rng, (V, hidden), kind)
                c = -(rng.integers(1, 65, size=V) / 64.0).astype(np.float32)
                set_lattice_head(enc, E, c)
                for lens in LENGTH_SETS + [short_seqs()]:
                    rows, cu = planted_case(rng, lens, E, c, kind)
                    want = truth(rows, cu, E, c)
                    got = enc.vocab_max(rows, cu)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (V, kind, lens[:4], np.abs(got - want).max())
                    if len(lens) > 2 and not all(n == lens[0] for n in lens) and len(lens) < 10:
                        assert not want[2].any() and want[0].any()   # the all-negative sequence, and one that is not
                # a small call after the large ones sees no stale maxima, and a second call gives the same bits
                rows, cu = planted_case(rng, [2], E, c, kind)
                a, b = enc.vocab_max(rows, cu), enc.vocab_max(rows, cu)
                assert np.array_equal(a.view(np.uint32), truth(rows, cu, E, c).view(np.uint32))
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        finally:
            enc.close()


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_vocab_max_full_vocabulary(mode):
    """V = 30522 = 119 * 256 + 58 (a partial column tile) with sequences that straddle the row tiles."""
    hidden, V = 384, 30522
    rng = np.random.default_rng(17)
    enc = make_encoder(hidden, mode, V)
    try:
        E = lattice(rng, (V, hidden), "eighths")
        c = -(rng.integers(1, 65, size=V) / 64.0).astype(np.float32)
        set_lattice_head(enc, E, c)
        rows, cu = planted_case(rng, [3, 250, 3, 300], E, c, "eighths")
        want = truth(rows, cu, E, c)
        got = enc.vocab_max(rows, cu)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(enc.vocab_max(rows, cu).view(np.uint32), got.view(np.uint32))
    finally:
        enc.close()


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("hidden,V", [(384, 314), (768, 58), (384, 1082)])
def test_topm_ties_and_padding(hidden, V, mode):
    """Top-m through the forward pass on a lattice head whose decoder rows repeat: repeated rows give exactly equal
    logits whatever g is, so ties straddle rank m and must go to the lower term id; V = 58 < m pads."""
    rng = np.random.default_rng(V)
    enc = make_encoder(hidden, mode, V)
    try:
        distinct = lattice(rng, (12, hidden), "eighths")
        group = rng.integers(0, 12, size=V)
        E = distinct[group]
        c = (-(rng.integers(1, 5, size=12) / 64.0).astype(np.float32))[group]
        set_lattice_head(enc, E, c)
        batch = [rng.integers(1, V, size=n).tolist() for n in (1, 5, 17, 40)]   # (never the pad id 0)
        for m in (1, 7, 256, 512):
            terms, weights, nnz, z = enc.encode_sparse_ids(batch, m, return_dense=True)
            assert (z >= 0).all()
            ties = 0
            for b in range(len(batch)):
                t_ref, w_ref, n_ref = sr.topm(z[b], m)
                assert nnz[b] == n_ref and np.array_equal(terms[b], t_ref), (m, b)
                # one fp32 unit in the last place of float64 log1p (the fp64 function's error is far below a half-ulp)
                assert np.all(np.abs(weights[b].view(np.int32) - w_ref.view(np.int32)) <= 1), (m, b)
                k = min(m, n_ref)
                if k < n_ref:
                    ties += int(z[b][t_ref[k - 1]] == np.sort(z[b])[::-1][k])
                if k < m:
                    assert (terms[b, k:] == -1).all() and (weights[b, k:] == 0).all()
            if V > 58 and m in (1, 7):
                assert ties > 0, "no tie straddles the cut: the case does not bind"
            if m > V:
                assert (nnz < m).all()
    finally:
        enc.close()
