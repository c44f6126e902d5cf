"""GPU: the fixed-dimensional encoding (css_fde_encode, csrc/css_fde.h) against its float64 restatement ``fde_numpy``:
bit for bit on lattice matrices, within the derived bounds on Gaussian ones, the same bytes whatever the batch and the
form, and through the index (``add_fde`` / ``search_fde``)."""
import numpy as np
import pytest

import late_cases as late
import lattice_cases as lc
from claude_semantic_search_amd import _native as nat
from claude_semantic_search_amd.flat_index import IndexFlatIP
from claude_semantic_search_amd.late_interaction import bf16_to_f32
from claude_semantic_search_amd.muvera import FixedDimensionalEncoding, fde_numpy

pytestmark = pytest.mark.gpu

LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 512)
CONFIGS = ((1, 16, 1), (3, 16, 5), (5, 16, 16), (6, 64, 2), (4, 32, 3))
EPS = 2.0 ** -24


def lattice_batch(P):
    return [lc.FAMILIES[f](m, P, 7 + i + 100 * j) for j, f in enumerate("TE") for i, m in enumerate(LENS)]


def csr(mats):
    off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    return off, np.concatenate(mats).astype(np.float64)


@pytest.mark.parametrize("is_query", (False, True))
@pytest.mark.parametrize("k_sim,d_proj,reps", CONFIGS)
@pytest.mark.parametrize("P", (32, 96, 128))
def test_lattice_exact(P, k_sim, d_proj, reps, is_query):
    """Every product and partial sum is exact, so ``out`` and the buckets are float64's with no tolerance.  The batch
    holds a dot that is exactly 0, a bucket of more than 32 tokens and an empty bucket filled through a Hamming tie.
    Two exemptions, for what these inputs cannot give (recomputed on the CPU for all 15 cases): at k_sim = 6 the 512
    tokens spread over 64 buckets and the fullest holds 18 .. 23; with ONE plane (k_sim = 1) a matrix of 15 or more
    tokens leaves neither bucket empty and the 1-token matrix has nobody to tie with."""
    mats = lattice_batch(P)
    off, tok = csr(mats)
    planes = lc.family_T(reps * k_sim, P, 5)
    proj = (np.random.default_rng(6).integers(0, 2, size=(reps * d_proj, P)) * 2 - 1).astype(np.float32)
    want, want_bk = fde_numpy(planes, proj, k_sim, d_proj, off, tok, is_query)
    assert (tok @ planes.T.astype(np.float64) == 0).any()
    B, tie, big = 1 << k_sim, False, False
    for i in range(len(mats)):
        for col in want_bk[off[i]:off[i + 1]].astype(np.int64).T:
            cnt = np.bincount(col, minlength=B)
            big |= bool(cnt.max(initial=0) > 32)
            for e in np.flatnonzero(cnt == 0)[:col.size]:
                ham = np.array([bin(int(v) ^ int(e)).count("1") for v in col])
                tie |= bool((ham == ham.min()).sum() > 1)
    assert big or k_sim == 6
    assert tie or k_sim == 1
    with FixedDimensionalEncoding(P, k_sim, d_proj, reps, planes=planes, proj=proj) as fde:
        assert fde.dim == reps * B * d_proj
        got, bk = fde._encode(mats, None, is_query, True, "test")
    assert np.array_equal(bk, want_bk)
    assert np.array_equal(got, want.astype(np.float32))
    assert not got[0].any() and not got[len(LENS)].any()   # the matrices without tokens


@pytest.mark.parametrize("is_query", (False, True))
@pytest.mark.parametrize("k_sim,d_proj,reps", ((5, 16, 16), (4, 32, 8)))
@pytest.mark.parametrize("P", (96, 128))
def test_gaussian_within_bounds(P, k_sim, d_proj, reps, is_query):
    """Default material, unit Gaussian rows rounded to bf16.  A bit may differ from float64's only inside the margin
    P 2^-24 sum |x_p plane_p| (and fewer than 1 dot in 1000 lies there: a condition on the inputs, asserted); every
    element lies within (cnt + P + 2) 2^-24 sum_p |proj_jp| sum_t |x_tp| / cnt of float64 on the DEVICE's buckets."""
    q, d = late.gaussian_mats(P, 11)
    mats = q + d
    off, tok = csr(mats)
    with FixedDimensionalEncoding(P, k_sim, d_proj, reps, seed=3) as fde:
        got, bk = fde._encode(mats, None, is_query, True, "test")
        planes, proj = bf16_to_f32(fde.planes).astype(np.float64), bf16_to_f32(fde.proj).astype(np.float64)
    dots, margin = tok @ planes.T, P * EPS * (np.abs(tok) @ np.abs(planes).T)
    sure = np.abs(dots) > margin
    assert (~sure).mean() < 1e-3
    dev_bits = (bk[:, :, None] >> np.arange(k_sim)) & 1
    assert np.array_equal(dev_bits.reshape(sure.shape)[sure], (dots > 0)[sure])
    want, _ = fde_numpy(planes, proj, k_sim, d_proj, off, tok, is_query, buckets=bk)
    B = 1 << k_sim
    bound = np.zeros((len(mats), reps, B, d_proj))
    for i in range(len(mats)):
        x, b = np.abs(tok[off[i]:off[i + 1]]), bk[off[i]:off[i + 1]].astype(np.int64)
        for r in range(reps):
            onehot = b[:, r, None] == np.arange(B)[None, :]
            cnt, S = onehot.sum(axis=0), onehot.T.astype(np.float64) @ x
            if not is_query:
                for e in np.flatnonzero(cnt == 0):   # a filled bucket holds the ONE token fde_numpy chose
                    ham = np.array([bin(int(v) ^ int(e)).count("1") for v in b[:, r]])
                    S[e] = x[int(ham.argmin())]
                cnt = np.maximum(cnt, 1)
            scale = (cnt + P + 2) * EPS / (1 if is_query else cnt)
            bound[i, r] = (S @ np.abs(proj[r * d_proj:(r + 1) * d_proj]).T) * scale[:, None]
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound.reshape(err.shape)).all(), float((err - bound.reshape(err.shape)).max())


def test_same_bytes_whatever_the_batch_and_the_form():
    mats = lattice_batch(96) + late.gaussian_mats(96, 5)[1]
    with FixedDimensionalEncoding(96, 4, 32, 3, seed=2) as fde:
        whole = fde.encode_documents(mats)
        assert np.array_equal(fde.encode_documents(mats[::-1])[::-1], whole)
        for i in (1, 5, 11, len(mats) - 1):
            assert np.array_equal(fde.encode_documents([mats[i]])[0], whole[i])
            assert np.array_equal(fde.encode_queries([mats[i]])[0], fde.encode_queries(mats)[i])
        assert np.array_equal(fde.encode_documents_dev(mats).cpu().numpy(), whole)
        assert np.array_equal(fde.encode_queries_dev(mats).cpu().numpy(), fde.encode_queries(mats))
        keep = late.keep_variants(mats)
        dropped = [m[k != 0] for m, k in zip(mats, keep)]
        assert np.array_equal(fde.encode_documents(mats, keep=keep), fde.encode_documents(dropped))


def test_add_fde_then_search_fde():
    qt, dt = late.lattice_mats("T", 32, 40)
    qe, de = late.lattice_mats("E", 32, 41)
    docs, queries = dt + de, qt + qe
    with FixedDimensionalEncoding(32, 3, 16, 2, seed=1) as fde:
        ix = IndexFlatIP(fde.dim)
        ix.add_fde(fde, docs[:5])
        ix.add_fde(fde, docs[5:])
        assert ix.ntotal == ix.token_rows == len(docs)
        off, tok = ix.get_tokens()
        assert np.array_equal(off, csr(docs)[0]) and np.array_equal(bf16_to_f32(tok), np.concatenate(docs))
        assert np.array_equal(ix.reconstruct_n(), fde.encode_documents(docs))
        for fetch in (4, len(docs)):
            got = ix.search_fde(fde, queries, 3, fetch)
            ref = ix.search_rerank_maxsim(fde.encode_queries(queries), queries, 3, fetch, normalize=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref))
        D, I = ix.search_maxsim_batch(queries, 3)
        assert np.array_equal(got[0], D) and np.array_equal(got[1], I)
        with pytest.raises(ValueError, match="dim="):
            IndexFlatIP(64).add_fde(fde, docs[:1])
        other = IndexFlatIP(fde.dim)   # a refusal that set_tokens would make comes BEFORE the rows are appended
        other.add(np.zeros((1, fde.dim), np.float32))
        other.set_tokens([np.ones((2, 64), np.float32)])
        with pytest.raises(ValueError, match="P=64"):
            other.add_fde(fde, docs[:1])
        assert other.ntotal == other.token_rows == 1
        other.close()
        ix.add(np.zeros((1, fde.dim), np.float32))
        with pytest.raises(ValueError, match="token matrices"):
            ix.add_fde(fde, docs[:1])
        ix.close()


@pytest.mark.parametrize("is_query,kind", ((0, "document"), (1, "query matrix")))
@pytest.mark.parametrize("off,bad,word", [
    ([1, 3, 5], None, "offsets start at 1"), ([0, 3, 2], None, "offsets decrease at {kind} 1"),
    ([0, 2, 515], None, "{kind} 1 has 513 tokens (at most 512)"),
    ([0, 2, 5], (3, 7, 0x7FC0), "component 7 of token 1 of {kind} 1 is NaN"),
    ([0, 2, 5], (0, 31, 0xFF80), "component 31 of token 0 of {kind} 0 is infinite")])
def test_library_refusals_name_the_matrix_and_write_nothing(off, bad, word, is_query, kind):
    """``tokens_as_csr`` refuses these first in Python, so the library's own checks are reached through ctypes."""
    off = np.array(off, dtype=np.int64)
    tok = np.zeros((max(int(off.max()), 1), 32), dtype=np.uint16)
    if bad:
        tok[bad[0], bad[1]] = bad[2]
    with FixedDimensionalEncoding(32, 2, 16, 1) as fde:
        out = np.full((2, fde.dim), 7.0, dtype=np.float32)
        rc = nat.lib().css_fde_encode(fde._handle(), off.ctypes.data, tok.ctypes.data, 2, is_query, out.ctypes.data, None)
        assert rc == nat.CSS_ERR_INVALID and word.format(kind=kind) in nat.last_error()
        assert (out == 7.0).all()
        assert fde.encode_documents([np.ones((3, 32), np.float32)]).shape == (1, fde.dim)   # the encoder stays usable
