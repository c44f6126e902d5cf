"""GPU: css_encoder_maxsim on lattice token matrices (tests/late_cases.py) -- every product and sum is exact in fp32,
so the scores must EQUAL the float64 truth bit for bit: no tolerance."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

from claude_semantic_search_amd.mpnet_encoder import MpnetEncoder

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import bert_reference as br  # noqa: E402
import late_cases as lt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    """Any encoder handle serves css_encoder_maxsim: the smallest one."""
    cfg = br.BertCfg(num_layers=1, vocab=1000, **br.SMALL)
    e = MpnetEncoder(synthetic_seed=1, cfg_overrides=cfg.encoder_overrides())
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _mats(family, P):
    q, d = lt.lattice_mats(family, P, seed=77 + P)
    return q, d, [lt.to_bf16(m) for m in q], [lt.to_bf16(m) for m in d]


def _equal(got, want32, what):
    assert got.dtype == np.float32 and got.shape == want32.shape
    bad = np.flatnonzero(got.view(np.uint32) != want32.view(np.uint32))
    print(f"[maxsim lattice] {what}: {got.size} scores, {bad.size} differ")
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want32[bad[:8]])


@pytest.mark.parametrize("P", lt.WIDTHS)
@pytest.mark.parametrize("family", ["T", "E"])
def test_all_pairs_equal_the_float64_truth(enc, family, P):
    q, d, qb, db = _mats(family, P)
    pairs = [(i, j) for i in range(len(q)) for j in range(len(d))]
    t64, t32 = lt.truth(q, d, pairs)
    assert np.array_equal(t32.astype(np.float64), t64)          # the truth itself is an fp32 number
    out = enc.maxsim(qb, db)
    _equal(out, t32, f"{family} P={P} all pairs")
    _equal(enc.maxsim(qb, db), out, f"{family} P={P} second call")


@pytest.mark.parametrize("P", lt.WIDTHS)
def test_keep_variants_equal_the_float64_truth(enc, P):
    q, d, qb, db = _mats("E", P)
    keep = lt.keep_variants(d)
    pairs = [(i, j) for i in range(len(q)) for j in range(len(d))]
    t64, t32 = lt.truth(q, d, pairs, keep)
    plain = lt.truth(q, d, pairs)[0]
    assert np.count_nonzero(t64 != plain) >= len(q)              # the flags change scores: the check is not vacuous
    _equal(enc.maxsim(qb, db, keep=keep), t32, f"E P={P} keep")


@pytest.mark.parametrize("P", lt.WIDTHS)
def test_pairs_repeated_reversed_and_sparse(enc, P):
    q, d, qb, db = _mats("T", P)
    pairs = lt.scrambled_pairs(len(q), len(d), skip_q=2, skip_d=3)
    assert all(i != 2 and j != 3 for i, j in pairs) and len(set(pairs)) < len(pairs)
    _, t32 = lt.truth(q, d, pairs)
    out = enc.maxsim(qb, db, pairs=pairs)
    _equal(out, t32, f"T P={P} scrambled pairs")
    assert enc.maxsim(qb, db, pairs=[]).shape == (0,)            # np == 0 is allowed


@pytest.mark.parametrize("count", [200, 600])
@pytest.mark.parametrize("P", [32, 128, 768])
def test_every_split_of_a_doc_over_blocks_gives_the_same_bits(enc, P, count):
    """The launcher spreads a doc over up to 8 blocks while the pairs alone do not fill the device: the 48 pairs of
    the other tests take 8 blocks per doc, 200 pairs a few, 600 pairs one block per doc (256 CUs).  All must return
    the truth's bits, with and without keep flags."""
    q, d, qb, db = _mats("E", P)
    base = lt.scrambled_pairs(len(q), len(d), skip_q=1, skip_d=0)
    pairs = (base * (count // len(base) + 1))[:count]
    keep = lt.keep_variants(d)
    for kp in (None, keep):
        _, t32 = lt.truth(q, d, base, kp)
        want = np.concatenate([t32] * (count // len(base) + 1))[:count]
        _equal(enc.maxsim(qb, db, pairs=pairs, keep=kp), want, f"E P={P} {count} pairs keep={kp is not None}")


@pytest.mark.parametrize("P", lt.WIDTHS)
def test_maximum_in_the_last_token_of_a_partial_tile(enc, P):
    """Doc of 17 and of 65 tokens whose LAST token (alone in its tile) copies a query row: dot(q, q) = the number of
    non-zero components, which no other {-1, 0, 1} row reaches unless it agrees on all of them."""
    q, d, _, _ = _mats("T", P)
    qm = q[3]                                                    # 17 query tokens
    for n in (17, 65):
        dm = np.array(d[lt.DOC_LENS.index(n)], copy=True)
        dm[-1] = qm[5]
        sim = qm.astype(np.float64) @ dm.astype(np.float64).T
        assert sim[5].argmax() == n - 1 and np.count_nonzero(sim[5] == sim[5].max()) == 1
        _, t32 = lt.truth([qm], [dm], [(0, 0)])
        _equal(enc.maxsim([lt.to_bf16(qm)], [lt.to_bf16(dm)]), t32, f"T P={P} doc {n}")


@pytest.mark.parametrize("P", lt.WIDTHS)
def test_negative_maxima(enc, P):
    """One query token of all ones against docs whose tokens have components in {-1, 0} with at least one -1: every dot
    is negative, so an accumulator that starts at 0, or a masked slot that enters as 0, returns 0 instead."""
    rng = np.random.default_rng(5 + P)
    qm = np.ones((1, P), dtype=np.float32)
    docs = []
    for n in (1, 15, 17, 65):
        dm = -rng.integers(0, 2, size=(n, P)).astype(np.float32)
        dm[:, 0] = -1.0
        docs.append(dm)
    pairs = [(0, j) for j in range(len(docs))]
    t64, t32 = lt.truth([qm], docs, pairs)
    assert (t64 < 0).all()
    _equal(enc.maxsim([lt.to_bf16(qm)], [lt.to_bf16(m) for m in docs]), t32, f"P={P} negative maxima")
