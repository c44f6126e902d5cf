"""GPU: ``IndexFlat.search_diverse`` (``css_index_search_diverse``, kernel ``k_mmr_select``) -- k rows picked by maximal
marginal relevance from the pool of the ``fetch`` best rows.

Three kinds of evidence.

(i)   ``lam = 1`` must be ``search(q, k)`` bit for bit.  Rows and queries are multiples of 1/8 (``tests/related_fakes.py``
      says why): every score is exact in float32 whatever kernel and summation order formed it, so the search for
      ``fetch`` rows and the search for ``k`` rows agree in every bit although they may take different kernels, and a
      third of the rows are copies, so the tie rule is exercised.
(ii)  Copies: every original stored three times.  A copy of a picked row has ``v`` at least 0.25 below any fresh row
      (checked in float64 on the data, not assumed), so no rounding decides -- the picks must come from distinct
      originals, in every search mode.
(iii) Clustered rows against float64: every pick must be a pool entry with the pool's score, the first pick the pool's
      first, and at every step the float64 value of the pick must reach the float64 maximum over the unpicked pool up to
      ``tol = 8 * (d + 2) * 2^-24 * M`` (``M`` the largest ``||x||^2`` / ``||q||^2``): the textbook fp32 dot-product
      bound on the two similarity sums that a comparison of two candidates involves.  Not a measured number, and not an
      exact-equality check either: float64 gaps between the two best candidates go down to 1e-6 on such data.

n 50 / 1000 (fewer rows than a pool, more than one), d 6 / 100 / 768 / 770 (6 and 770 are no multiples of 4: the scalar
row loop; 770 pads to another row pitch), nq 1 / 5 / 70."""
import ctypes

import numpy as np
import pytest

from knn_checks import SCORE_TOL

pytestmark = pytest.mark.gpu

NS = (50, 1000)
DS = (6, 100, 768, 770)
NQS = (1, 5, 70)
FLT_MAX = np.finfo(np.float32).max


def _pad(metric):
    return -FLT_MAX if metric == 0 else FLT_MAX


def _index(d, metric, x, shadow=None, id_base=0, mode=None, reserve=0):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(shadow)
    if id_base:
        ix.set_id_base(id_base)
    if reserve:
        ix.reserve(reserve)
    if x.shape[0]:
        ix.add(x)
    if mode:
        ix.set_search_mode(mode)
    return ix


def _eighths(n, d, seed, copies=True):
    x = (np.random.default_rng(seed).integers(-8, 9, size=(n, d)) / 8.0).astype(np.float32)
    if copies and n >= 3:
        x[n - n // 3:] = x[:n // 3]
    return x


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ at {np.argwhere(got[1] != want[1])[:5].tolist()}"
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: scores differ"


_CLUSTERED = {}


def _clustered(n, d, seed, norms=False):
    """12 unit centres; a row is its centre plus Gaussian noise of total length ~0.3 (0.3 / sqrt(d) per coordinate),
    renormalised; ``norms``: rows then scaled to lengths in [0.5, 2].  Computed once per shape and left unchanged."""
    key = (n, d, seed, norms)
    if key not in _CLUSTERED:
        rng = np.random.default_rng(seed)
        c = rng.standard_normal((12, d))
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        x = c[rng.integers(0, 12, size=n)] + 0.3 / np.sqrt(d) * rng.standard_normal((n, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        if norms:
            x *= rng.uniform(0.5, 2.0, size=(n, 1))
        x = x.astype(np.float32)
        x.setflags(write=False)
        _CLUSTERED[key] = x
    return _CLUSTERED[key]


def _queries(x, nq, seed):
    """Queries near stored rows (a search that has near-copies to push apart), unit length."""
    rng = np.random.default_rng(seed)
    q = x[rng.integers(0, x.shape[0], size=nq)].astype(np.float64) + 0.2 / np.sqrt(x.shape[1]) * rng.standard_normal((nq, x.shape[1]))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------ (i) lam = 1 is search(q, k)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("metric", [0, 1])
def test_lam_one_is_the_plain_search_bit_for_bit(metric, d, n):
    x = _eighths(n, d, 3 + d)
    q = _eighths(max(NQS), d, 1000 + d, copies=False)
    ix = _index(d, metric, x)
    for nq in NQS:
        for k in (1, 10, 32, 128):
            want = ix.search(q[:nq], k)
            for fetch in (0, 32, 128):
                if k <= (fetch or 128):
                    _same(ix.search_diverse(q[:nq], k, lam=1.0, fetch=fetch), want, f"metric={metric} d={d} n={n} nq={nq} k={k} fetch={fetch}")
    ix.close()


# ------------------------------------------------------------------------------------------------------------ (ii) copies
def _copies_data():
    rng = np.random.default_rng(8)
    base = rng.standard_normal((40, 768))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    order = rng.permutation(120)                         # id i holds original order[i] % 40
    x = base[order % 40].astype(np.float32)
    q = rng.standard_normal((5, 768))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return x, q, order % 40


def _copies_margins(x, q, metric):
    """float64: the largest value a copy of a picked row can have, the smallest a fresh row can have (lam = 0.5)."""
    x64, q64 = x[:40 * 3].astype(np.float64), q.astype(np.float64)
    if metric == 0:
        rel, sim = q64 @ x64.T, x64 @ x64.T
        same = 1.0 - 1e-6
    else:
        rel = -((q64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
        sim = -((x64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
        same = -1e-6
    copy = sim >= same                                   # pairs of copies (and a row with itself)
    fresh_lo = 0.5 * rel.min() - 0.5 * sim[~copy].max()
    copy_hi = 0.5 * rel.max() - 0.5 * sim[copy].min()
    return copy_hi, fresh_lo


@pytest.mark.parametrize("metric", [0, 1])
def test_copies_are_pushed_behind_every_fresh_row(metric):
    x, q, orig = _copies_data()
    copy_hi, fresh_lo = _copies_margins(x, q, metric)
    assert fresh_lo - copy_hi > 0.25                     # IP: fresh >= -0.15, copy <= -0.42; L2 wider still
    want_I = None
    for mode, shadow in (("exact_fp32", None), ("coarse", None), ("auto", None), ("auto", False)):
        ix = _index(768, metric, x, shadow=shadow, mode=mode)
        D, I = ix.search_diverse(q, 20, lam=0.5, fetch=128)
        Dp, Ip = ix.search(q, 128)
        for j in range(q.shape[0]):
            assert (I[j] >= 0).all() and len(set(orig[I[j]].tolist())) == 20, f"{mode} shadow={shadow} query {j}: a copy was picked"
            assert I[j, 0] == Ip[j, 0]
            pos = [int(np.flatnonzero(Ip[j] == i)[0]) for i in I[j]]
            assert np.array_equal(D[j].view(np.uint32), Dp[j, pos].view(np.uint32))
        # The same picks whatever path formed the pool.  Paths differ only in the last bits of the pool's scores
        # (<= 1e-6, css_hip.h); the similarities come from the stored rows and one kernel.  So v moves by <= 1e-6
        # between paths, and no step of this data is within 2e-5 of a tie between originals (checked in float64)
        if want_I is None:
            want_I = I
            _assert_wide_steps(x, q, I, orig, metric, 0.5, 2e-5)
        assert np.array_equal(I, want_I), f"{mode} shadow={shadow}"
        # 40 originals are all there is: k = 60 picks every original once before any copy
        D, I = ix.search_diverse(q[:1], 60, lam=0.5, fetch=128)
        assert len(set(orig[I[0, :40]].tolist())) == 40
        ix.close()


def _sim64(rows, p, metric):
    """float64 similarity of every row of ``rows`` to the row ``p``."""
    return rows @ p if metric == 0 else -((rows - p[None, :]) ** 2).sum(-1)


def _assert_wide_steps(x, q, I, orig, metric, lam, gap):
    """No step of the pick sequence ``I`` was a near tie between ORIGINALS: in float64 the pick's value is more than
    ``gap`` away from the best row of any other original, and among the (exactly tied) copies of its own original the
    pick has the lowest id."""
    x64 = x.astype(np.float64)
    for j in range(q.shape[0]):
        rel = _sim64(x64, q[j].astype(np.float64), metric)
        pen = np.full(x.shape[0], -np.inf)
        for t in range(1, I.shape[1]):
            pen = np.maximum(pen, _sim64(x64, x64[I[j, t - 1]], metric))
            v = lam * rel - (1.0 - lam) * pen
            v[I[j, :t]] = -np.inf
            mine = orig == orig[I[j, t]]
            assert abs(v[I[j, t]] - v[~mine].max()) > gap, (j, t)
            assert I[j, t] == np.flatnonzero(mine & (v > -np.inf))[0], (j, t)


# ------------------------------------------------------------------------------------------- (iii) float64 path check
def _check_path(ix, x, q, metric, k, fetch, lam, what, allow=None, id_base=0):
    d = x.shape[1]
    Dp, Ip = ix.search(q, fetch or (32 if 4 * k <= 32 else 128), allow=allow)   # (fetch = 0: the automatic pool)
    D, I = ix.search_diverse(q, k, lam=lam, fetch=fetch, allow=allow)
    x64 = x.astype(np.float64)
    M = max(float((x64 ** 2).sum(1).max()), float((q.astype(np.float64) ** 2).sum(1).max()))
    tol = 8.0 * (d + 2) * 2.0 ** -24 * M
    worst = 0.0
    for j in range(q.shape[0]):
        mv = int((Ip[j] >= 0).sum())
        npk = min(k, mv)
        assert (I[j, npk:] == -1).all() and (D[j, npk:] == _pad(metric)).all(), f"{what}: query {j}: padding"
        assert (I[j, :npk] >= 0).all() and len(set(I[j, :npk].tolist())) == npk, f"{what}: query {j}: repeated or missing picks"
        if npk == 0:
            continue
        pos = []
        for i in I[j, :npk]:
            at = np.flatnonzero(Ip[j] == i)
            assert at.size == 1, f"{what}: query {j}: id {i} is not in the pool"
            pos.append(int(at[0]))
        assert np.array_equal(D[j, :npk].view(np.uint32), Dp[j, pos].view(np.uint32)), f"{what}: query {j}: D is not the pool's score"
        assert pos[0] == 0, f"{what}: query {j}: the first pick is not the pool's first"
        rows = x64[Ip[j, :mv] - id_base]
        rel = Dp[j, :mv].astype(np.float64) if metric == 0 else -Dp[j, :mv].astype(np.float64)   # (rel is the fp32 score, as defined)
        pen = np.full(mv, -np.inf)
        for t in range(1, npk):
            pen = np.maximum(pen, _sim64(rows, rows[pos[t - 1]], metric))
            v = lam * rel - (1.0 - lam) * pen
            v[pos[:t]] = -np.inf
            short = float(v.max() - v[pos[t]])
            worst = max(worst, short)
            assert short <= tol, f"{what}: query {j} step {t}: pick {I[j, t]} is {short:.3e} below the best (tol {tol:.3e})"
    print(f"{what}: largest float64 shortfall {worst:.3e}, tol {tol:.3e}")


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("kind", ["ip_unit", "ip_norms", "l2_unit"])
def test_every_pick_is_the_float64_best_within_the_fp32_bound(kind, d):
    metric = 1 if kind == "l2_unit" else 0
    x = _clustered(1000, d, 100 + d, norms=kind == "ip_norms")
    q = _queries(x, max(NQS), 200 + d)
    ix = _index(d, metric, x)
    for nq, k, fetch, lam in ((1, 10, 128, 0.5), (5, 10, 0, 0.3), (70, 10, 128, 0.7), (5, 8, 0, 0.5), (5, 32, 32, 0.5), (1, 40, 128, 0.0)):
        _check_path(ix, x, q[:nq], metric, k, fetch, lam, f"{kind} d={d} nq={nq} k={k} fetch={fetch} lam={lam}")
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_k_equal_to_fetch_returns_a_permutation_of_the_pool(metric):
    d = 100
    x = _clustered(1000, d, 100 + d)
    q = _queries(x, 5, 300)
    ix = _index(d, metric, x)
    Dp, Ip = ix.search(q, 128)
    D, I = ix.search_diverse(q, 128, lam=0.5, fetch=128)
    assert np.array_equal(np.sort(I, axis=1), np.sort(Ip, axis=1)) and (I >= 0).all()
    assert not np.array_equal(I, Ip)                     # ... and not the identity on clustered rows
    _check_path(ix, x, q, metric, 128, 128, 0.5, f"k = fetch = 128 metric={metric}")
    ix.close()


# -------------------------------------------------------------------------------------------------------- short pools
@pytest.mark.parametrize("d", [6, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_short_pools_are_padded(metric, d):
    x = _clustered(50, d, 400 + d)
    q = _queries(x, 5, 401)
    ix = _index(d, metric, x)
    D, I = ix.search_diverse(q, 128, lam=0.5, fetch=128)                 # 50 rows: 50 picks, then pads
    assert all(sorted(I[j, :50].tolist()) == list(range(50)) for j in range(5))
    assert (I[:, 50:] == -1).all() and (D[:, 50:] == _pad(metric)).all()
    _check_path(ix, x, q, metric, 128, 128, 0.5, f"n=50 metric={metric} d={d}")
    _check_path(ix, x, q, metric, 60, 128, 0.25, f"n=50 k=60 metric={metric} d={d}")
    allow = np.zeros(50, bool)
    allow[[1, 2, 3, 17, 31, 32, 49]] = True                              # 7 rows
    D, I = ix.search_diverse(q, 10, lam=0.5, allow=allow)
    assert all(sorted(I[j, :7].tolist()) == [1, 2, 3, 17, 31, 32, 49] for j in range(5))
    assert (I[:, 7:] == -1).all() and (D[:, 7:] == _pad(metric)).all()
    _check_path(ix, x, q, metric, 10, 128, 0.5, f"7 allowed rows metric={metric} d={d}", allow=allow)
    D, I = ix.search_diverse(q, 10, lam=0.5, allow=np.zeros(50, bool))   # nothing allowed
    assert (I == -1).all() and (D == _pad(metric)).all()
    D, I = ix.search_diverse(np.zeros((0, d), np.float32), 10)           # nq = 0
    assert D.shape == (0, 10) and I.shape == (0, 10) and D.dtype == np.float32 and I.dtype == np.int64
    ix.close()
    empty = _index(d, metric, x[:0])
    D, I = empty.search_diverse(q, 10, lam=0.5)
    assert (I == -1).all() and (D == _pad(metric)).all()
    empty.close()


# -------------------------------------------------------------------------------------------------------- index state
def test_id_base_moves_the_ids_only():
    d, base = 100, 5_000_000_000
    x = _clustered(1000, d, 100 + d)
    q = _queries(x, 5, 500)
    ix0 = _index(d, 0, x)
    ix = _index(d, 0, x, id_base=base)
    for k, fetch, lam in ((10, 0, 0.5), (32, 128, 0.25)):
        D0, I0 = ix0.search_diverse(q, k, lam=lam, fetch=fetch)
        D, I = ix.search_diverse(q, k, lam=lam, fetch=fetch)
        assert np.array_equal(I, I0 + base) and np.array_equal(D.view(np.uint32), D0.view(np.uint32))
    _check_path(ix, x, q, 0, 10, 128, 0.5, "id_base", id_base=base)
    ix0.close()
    ix.close()


def test_after_remove_ids_and_after_growth_the_index_answers_like_a_fresh_one():
    d = 770
    x = _clustered(1000, d, 100 + d)
    q = _queries(x, 5, 600)
    keep = np.random.default_rng(601).random(1000) < 0.7
    ix = _index(d, 1, x)
    assert ix.remove_ids(np.flatnonzero(~keep)) == int((~keep).sum())
    fresh = _index(d, 1, x[keep])
    for k, fetch, lam in ((10, 0, 0.5), (32, 128, 0.25)):
        _same(ix.search_diverse(q, k, lam=lam, fetch=fetch), fresh.search_diverse(q, k, lam=lam, fetch=fetch), f"removed k={k}")
    _check_path(ix, x[keep], q, 1, 10, 128, 0.5, "after remove_ids")
    ix.close()
    fresh.close()
    grown = _index(d, 0, x[:300], reserve=300)
    D0, I0 = grown.search_diverse(q, 10, lam=0.5)                        # (workspaces sized before the growth)
    grown.add(x[300:])                                                   # 1000 rows > the 300 reserved: reallocated
    fresh = _index(d, 0, x)
    for k, fetch, lam in ((10, 0, 0.5), (32, 128, 0.25)):
        _same(grown.search_diverse(q, k, lam=lam, fetch=fetch), fresh.search_diverse(q, k, lam=lam, fetch=fetch), f"grown k={k}")
    _check_path(grown, x, q, 0, 10, 128, 0.5, "after growth")
    grown.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------------ the device twin
@pytest.mark.parametrize("metric", [0, 1])
def test_the_device_twin_on_a_side_stream_equals_the_host_call(metric):
    import torch

    from claude_semantic_search_amd.flat_index import pack_allow_bits

    d = 768
    x = _clustered(1000, d, 100 + d)
    q = _queries(x, 70, 700)
    ix = _index(d, metric, x)
    allow = np.random.default_rng(701).random(1000) < 0.5
    side = torch.cuda.Stream()
    qt = torch.from_numpy(q).cuda()
    bits = torch.from_numpy(pack_allow_bits(allow, 1000).view(np.int32)).cuda()
    torch.cuda.synchronize()
    for nq, k, fetch, lam, masked in ((70, 10, 128, 0.5, False), (5, 32, 32, 0.25, True), (1, 8, 0, 0.5, False)):
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        with torch.cuda.stream(side):
            ix.search_diverse_dev(qt.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), stream=side.cuda_stream, lam=lam,
                                  fetch=fetch, allow_bits_ptr=bits.data_ptr() if masked else 0)
        side.synchronize()
        want = ix.search_diverse(q[:nq], k, lam=lam, fetch=fetch, allow=allow if masked else None)
        _same((D.cpu().numpy(), I.cpu().numpy()), want, f"dev metric={metric} nq={nq} k={k}")
    ix.search_diverse_dev(0, 0, 3, 0, 0)                                 # nq = 0: a no-op, nothing is dereferenced
    ix.close()


# ---------------------------------------------------------------------------------------------------------- error codes
def test_error_codes_through_the_c_abi():
    from claude_semantic_search_amd import _native as nat

    d = 6
    x = _clustered(50, d, 406)
    ix = _index(d, 0, x)
    q = np.ascontiguousarray(x[:2])
    D, I = np.empty((2, 200), np.float32), np.empty((2, 200), np.int64)
    lib = nat.lib()

    def call(k, fetch, lam, nq=2):
        return lib.css_index_search_diverse(ix._handle(), q.ctypes.data, nq, k, fetch, ctypes.c_float(lam), 0, None,
                                            D.ctypes.data, I.ctypes.data)

    for k, fetch, lam, word in ((5, 0, -0.1, "lam="), (5, 0, 1.5, "lam="), (5, 0, float("nan"), "lam="), (33, 32, 0.5, "k="),
                                (129, 0, 0.5, "k="), (5, 129, 0.5, "fetch="), (5, -1, 0.5, "fetch="), (0, 0, 0.5, "k="),
                                (0, 32, 0.5, "k=")):
        assert call(k, fetch, lam) == nat.CSS_ERR_INVALID, (k, fetch, lam)
        assert word in nat.last_error() and "css_index_search_diverse" in nat.last_error(), nat.last_error()
        assert lib.css_index_search_diverse_dev(ix._handle(), None, 0, k, fetch, ctypes.c_float(lam), 0, None, None, None,
                                                None) == nat.CSS_ERR_INVALID
        assert word in nat.last_error()
    assert call(5, 0, 0.5, nq=-1) == nat.CSS_ERR_INVALID
    assert lib.css_index_search_diverse(None, q.ctypes.data, 2, 5, 0, ctypes.c_float(0.5), 0, None, D.ctypes.data,
                                        I.ctypes.data) == nat.CSS_ERR_INVALID
    assert lib.css_index_search_diverse(ix._handle(), None, 2, 5, 0, ctypes.c_float(0.5), 0, None, D.ctypes.data,
                                        I.ctypes.data) == nat.CSS_ERR_INVALID
    assert call(5, 0, 0.5, nq=0) == nat.CSS_OK                           # nq = 0: a no-op
    assert call(5, 0, 0.5) == nat.CSS_OK and call(1, 1, 0.0) == nat.CSS_OK and call(128, 128, 1.0) == nat.CSS_OK
    with pytest.raises(ValueError):                                      # the Python checks sit in front
        ix.search_diverse(q, 5, lam=1.5)
    ix.close()


# ------------------------------------------------------------------------------------------- HybridStorage on the index
@pytest.mark.parametrize("sharded", [False, True], ids=["one_index", "facade"])
@pytest.mark.parametrize("pushdown", [False, True])
def test_storage_returns_a_pasted_passage_once(tmp_path, pushdown, sharded):
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, SearchConfig, StorageConfig

    d = 768
    rng = np.random.default_rng(800)
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    raw = rng.standard_normal((30, d))
    raw /= np.linalg.norm(raw, axis=1, keepdims=True)
    for i in range(3, 30):                               # distinct chunks: cos to the query falling from 0.6 to 0.3
        c = 0.6 - 0.3 * (i - 3) / 26
        u = raw[i] - (raw[i] @ q) * q
        raw[i] = c * q + np.sqrt(1 - c * c) * u / np.linalg.norm(u)
    for i in range(3):                                   # one passage pasted into three sessions: cos 0.9
        u = raw[0] - (raw[0] @ q) * q
        raw[i] = 0.9 * q + np.sqrt(1 - 0.81) * u / np.linalg.norm(u) + 1e-4 * i * raw[29]
    order = rng.permutation(30)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path / "s"), embedding_dim=d, auto_save=False, filter_pushdown=pushdown,
                                    sharded=sharded))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", f"t{i}", {"project_name": "p", "has_code": int(i) % 2 == 0, "session_id": f"s{i}"},
                        raw[i].astype(np.float32)) for i in order])
    dup = {"c0", "c1", "c2"}
    plain = s.search(q.astype(np.float32), SearchConfig(top_k=5))
    assert {r.chunk_id for r in plain[:3]} == dup        # search(): the three copies lead
    res = s.search_diverse(q.astype(np.float32), SearchConfig(top_k=5))
    ids = [r.chunk_id for r in res]
    assert len(ids) == 5 and ids[0] == plain[0].chunk_id and not dup & set(ids[1:])
    by_id = {r.chunk_id: r.similarity for r in s.search(q.astype(np.float32), SearchConfig(top_k=30, max_results=30))}
    assert all(abs(r.similarity - by_id[r.chunk_id]) <= SCORE_TOL for r in res)      # the ordinary score of every pick
    # lam = 1: the order of search()
    assert [r.chunk_id for r in s.search_diverse(q.astype(np.float32), SearchConfig(top_k=5), lam=1.0)] == [r.chunk_id for r in plain]
    # a deleted copy neither comes back nor stands in the way: the next copy leads
    assert s.delete_chunk(plain[0].chunk_id)
    res = s.search_diverse(q.astype(np.float32), SearchConfig(top_k=5), filters={"project_name": "p"})
    ids = [r.chunk_id for r in res]
    assert ids[0] == plain[1].chunk_id and plain[0].chunk_id not in ids and len(dup & set(ids)) == 1
    s.close()
