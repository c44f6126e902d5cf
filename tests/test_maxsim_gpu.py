"""GPU: css_encoder_maxsim on Gaussian unit rows rounded to bf16 against float64 on the same bf16 values, and the
refusals of the late-interaction entry points (each before anything is enqueued, naming the offending item)."""
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
    cfg = br.BertCfg(num_layers=1, vocab=1000, **br.SMALL)
    e = MpnetEncoder(synthetic_seed=1, cfg_overrides=cfg.encoder_overrides())
    yield e
    e.close()


@pytest.mark.parametrize("P", lt.WIDTHS)
def test_gaussian_rows_within_the_derived_bound(enc, P):
    """|score - truth| <= 2^-23 m (P + m) c with m the query's tokens and c the largest ||q_s|| ||d_t|| of the pair: an
    fp32 dot of P exact products in any order errs by at most 2^-23 P c (c bounds every sum of |products|), a maximum
    moves by no more than its arguments, and each of the m - 1 fp32 additions of maxima of magnitude <= c adds at most
    2^-23 m c -- derived, not measured (the measured ratio to it is printed)."""
    q, d = lt.gaussian_mats(P, seed=900 + P)
    qb, db = [lt.to_bf16(m) for m in q], [lt.to_bf16(m) for m in d]
    keep = lt.keep_variants(d)
    worst = 0.0
    for kp in (None, keep):
        pairs = [(i, j) for i in range(len(q)) for j in range(len(d))]
        t64, _ = lt.truth(q, d, pairs, kp)
        out = enc.maxsim(qb, db, keep=kp)
        assert out.dtype == np.float32 and out.shape == t64.shape
        for n, (i, j) in enumerate(pairs):
            m = q[i].shape[0]
            c = float(np.linalg.norm(q[i].astype(np.float64), axis=1).max() *
                      np.linalg.norm(d[j].astype(np.float64), axis=1).max())
            bound = 2.0 ** -23 * m * (P + m) * c
            err = abs(float(out[n]) - t64[n])
            worst = max(worst, err / bound)
            assert err <= bound, (P, i, j, err, bound)
    print(f"[maxsim gaussian] P={P}: largest |score - truth| / bound = {worst:.3e}")


def test_refusals_name_the_offending_item(enc):
    ok_q = [np.zeros((3, 32), np.uint16)]
    ok_d = [np.zeros((5, 32), np.uint16), np.zeros((2, 32), np.uint16)]
    before = enc.maxsim(ok_q, ok_d)
    with pytest.raises(RuntimeError, match=r"P=48"):
        enc.maxsim([np.zeros((3, 48), np.uint16)], [np.zeros((5, 48), np.uint16)])
    with pytest.raises(RuntimeError, match=r"query 1 has 65 tokens"):
        enc.maxsim(ok_q + [np.zeros((65, 32), np.uint16)], ok_d)
    with pytest.raises(RuntimeError, match=r"doc 1 has no kept token"):
        enc.maxsim(ok_q, ok_d, keep=[np.ones(5, np.uint8), np.zeros(2, np.uint8)])
    with pytest.raises(RuntimeError, match=r"pair 1 is \(query 0, doc 2\)"):
        enc.maxsim(ok_q, ok_d, pairs=[(0, 0), (0, 2)])
    with pytest.raises(RuntimeError, match=r"pair 0 is \(query -1, doc 0\)"):
        enc.maxsim(ok_q, ok_d, pairs=[(-1, 0)])
    with pytest.raises(ValueError, match=r"d_mats\[0\] has P=64 columns, expected P=32"):
        enc.maxsim(ok_q, [np.zeros((5, 64), np.uint16)])
    # q_tok whose P differs from the encoder's (hidden 384, no projection)
    assert enc.token_dim == 384
    batch = br.synth_batch(br.BertCfg(num_layers=1, vocab=1000, **br.SMALL), [7, 4], 3)
    with pytest.raises(ValueError, match=r"q_mats\[0\] has P=32 columns, expected P=384"):
        enc.score_late_ids(batch, ok_q)
    with pytest.raises(RuntimeError, match=r"P=48"):
        enc.set_token_projection(np.zeros((48, 384), np.float32))
    with pytest.raises(RuntimeError, match=r"P=160"):
        enc.set_token_projection(np.zeros((160, 384), np.float32))
    with pytest.raises(ValueError, match=r"expected \[P, 384\]"):
        enc.set_token_projection(np.zeros((32, 768), np.float32))
    with pytest.raises(RuntimeError, match=r"doc 0 has no kept token"):
        enc.score_late_ids(batch, [np.zeros((3, 384), np.uint16)], keep=[np.zeros(7, np.uint8), np.ones(4, np.uint8)])
    assert enc.token_dim == 384                                   # a refused projection leaves the state alone
    assert np.array_equal(before, enc.maxsim(ok_q, ok_d))
