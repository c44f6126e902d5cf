"""GPU: ``IndexFlat.remove_ids`` (``css_index_remove_rows``) -- in-place stream compaction of the index rows.

The bar is bit equality with an index freshly built from the surviving rows (``add(np.delete(x, ids, 0))``): the same
fp32 rows give the same bf16 / int8 rows, the same three maxima (``bounds()``), hence the same error bands and the same
fixed-order rescoring, so ``D`` and ``I`` of every search mode must be identical.  The fresh index in turn is checked
against ``FlatIndexOracle`` on the survivors with the suite's usual comparison (``knn_checks``).

Pruning of metric x dim x shadow policy x pattern x n (everything else is covered):
  * all nine removal patterns run at (IP, 768, automatic shadow) for n = 70 001 (several row windows, bounced and
    direct ones) and on the small sizes 1..65 (word boundaries of the keep bitmap);
  * all 24 combinations of metric x dim x shadow policy run the random-10 % pattern at n = 50 000; the other patterns
    do not depend on metric or policy (the move treats every row alike), so they are not multiplied out;
  * n = 200 000 runs three patterns (every other row, random 10 %, random 90 %) at (IP, 768, automatic).
"""
import numpy as np
import pytest

from oracle import knn_oracle as ko
from knn_checks import assert_topk_matches

pytestmark = pytest.mark.gpu

PATTERNS = ("none", "all", "first", "last", "every_other", "random10", "random90", "block", "all_but_one")
POLICIES = {"off": False, "bf16": True, "int8": "int8", "auto": None}


def _ids(pattern, n, seed=5):
    rng = np.random.default_rng(seed)
    if pattern == "none":
        return np.zeros(0, np.int64)
    if pattern == "all":
        return np.arange(n, dtype=np.int64)
    if pattern == "first":
        return np.array([0], np.int64)
    if pattern == "last":
        return np.array([n - 1], np.int64)
    if pattern == "every_other":
        return np.arange(0, n, 2, dtype=np.int64)
    if pattern == "random10":
        return np.flatnonzero(rng.random(n) < 0.10).astype(np.int64)
    if pattern == "random90":
        return np.flatnonzero(rng.random(n) < 0.90).astype(np.int64)
    if pattern == "block":
        return np.arange(n // 3, max(n // 3 + 1, (2 * n) // 3), dtype=np.int64)
    if pattern == "all_but_one":
        return np.delete(np.arange(n, dtype=np.int64), n // 2)
    raise AssertionError(pattern)


def _rows(n, d, seed):
    return ko.normalize_rows(ko.synth_rows(n, d, seed))


def _index(d, metric, policy, x=None):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(POLICIES[policy])
    if x is not None and x.shape[0]:
        ix.add(x)
    return ix


def _bits(b):
    return np.array([b["max_norm2"], b["max_bf16_err2"], b["max_int8_err2"]], np.float32).view(np.uint32).tolist()


def _assert_same_as_fresh(ix, fresh, surv, metric, what, queries=(1, 4, 16, 300), ks=(10, 100), oracle=True, seed=77):
    """rows, maxima and every search of ``ix`` against ``fresh`` (bit for bit) and against the oracle on ``surv``."""
    m, d = surv.shape
    assert ix.ntotal == m == fresh.ntotal, what
    assert np.array_equal(ix.reconstruct_n(0, m).view(np.uint32), surv.view(np.uint32)), f"{what}: rows differ"
    assert _bits(ix.bounds()) == _bits(fresh.bounds()), f"{what}: bounds {ix.bounds()} != {fresh.bounds()}"
    assert ix.shadow_info() == fresh.shadow_info() or m == 0, what
    if m == 0:
        return
    q = _rows(max(queries), d, seed)
    ref = None
    if oracle:
        ref = ko.FlatIndexOracle(d, metric)
        ref.add(surv)
    for k in ks:
        if oracle:
            Dr, Ir = ref.search(q, k)
            D64 = ref.rescore64(q, np.where(Ir < 0, 0, Ir))
        for mode in ("exact_fp32", "coarse", "auto"):
            ix.set_search_mode(mode)
            fresh.set_search_mode(mode)
            for nq in queries:
                D, I = ix.search(q[:nq], k)
                Df, If = fresh.search(q[:nq], k)
                w = f"{what} [{mode}] nq={nq} k={k}"
                assert np.array_equal(I, If), f"{w}: ids differ from a freshly built index"
                assert np.array_equal(D.view(np.uint32), Df.view(np.uint32)), f"{w}: scores differ from a freshly built index"
                if oracle:
                    assert_topk_matches(D, I, Dr[:nq], Ir[:nq], D64[:nq], w)
    ix.set_search_mode("auto")
    fresh.set_search_mode("auto")


def _run(metric, d, policy, n, pattern, seed=1, **kw):
    x = _rows(n, d, seed)
    ids = _ids(pattern, n)
    surv = np.delete(x, ids, 0)
    ix = _index(d, metric, policy, x)
    removed = ix.remove_ids(ids)
    what = f"metric={metric} d={d} shadow={policy} n={n} {pattern}"
    assert removed == n - surv.shape[0], what
    fresh = _index(d, metric, policy, surv)
    _assert_same_as_fresh(ix, fresh, surv, metric, what, **kw)
    ix.close()
    fresh.close()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns_across_row_windows(pattern):
    _run(0, 768, "auto", 70001, pattern)


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65])
def test_patterns_on_small_indexes(n):
    for pattern in PATTERNS:
        _run(0, 384, "auto", n, pattern, ks=(10,), queries=(1, 16))


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("d", [100, 384, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_every_metric_dim_and_shadow_policy(metric, d, policy):
    _run(metric, d, policy, 50000, "random10")


@pytest.mark.parametrize("pattern", ["every_other", "random10", "random90"])
def test_200k_rows(pattern):
    _run(0, 768, "auto", 200000, pattern, ks=(10,))


def test_mask_form_and_ignored_ids():
    n, d = 5000, 384
    x = _rows(n, d, 3)
    ix = _index(d, 0, "auto", x)
    assert ix.remove_ids([]) == 0 and ix.remove_ids([n, -1, 10 ** 15]) == 0 and ix.ntotal == n
    assert ix.remove_ids([7, 7, 7, n + 3, 4999]) == 2
    surv = np.delete(x, [7, 4999], 0)
    mask = np.zeros(n - 2, bool)
    mask[100:200] = True
    assert ix.remove_ids(mask) == 100
    surv = np.delete(surv, np.arange(100, 200), 0)
    fresh = _index(d, 0, "auto", surv)
    _assert_same_as_fresh(ix, fresh, surv, 0, "mask form", ks=(10,))
    with pytest.raises(ValueError):
        ix.remove_ids(np.zeros(n, bool))
    with pytest.raises(ValueError):
        ix.remove_ids([1.5])
    assert ix.remove_ids(np.ones(ix.ntotal, bool)) == n - 102 and ix.ntotal == 0
    assert ix.remove_ids([0]) == 0                                   # empty index
    assert _bits(ix.bounds()) == [0, 0, 0]
    ix.add(x[:10])                                                    # an emptied index takes rows again
    assert np.array_equal(ix.reconstruct_n(0, 10), x[:10])
    ix.close()
    fresh.close()


@pytest.mark.parametrize("where", ["moved part", "unmoved prefix"])
def test_maxima_shrink_when_the_outlier_rows_leave(where):
    """Row `big` has by far the largest norm, row `coarse8` (unit norm, one dominant element) by far the largest int8
    error: while they are in the index they set the maxima, once removed the maxima are those of the survivors."""
    n, d = 30000, 768
    x = _rows(n, d, 9)
    big, coarse8 = (20000, 25000) if where == "moved part" else (10, 20)
    x[big] *= 3.0
    x[coarse8] *= 0.3
    x[coarse8, 5] = 0.0
    x[coarse8, 5] = np.sqrt(1.0 - float((x[coarse8].astype(np.float64) ** 2).sum()))
    ix = _index(d, 0, "auto", x)
    b0 = ix.bounds()
    assert b0["max_norm2"] > 8.5
    first_removed = 15000 if where == "moved part" else 15   # (prefix case: row `big` stays where it is)
    # (1) only the int8 outlier leaves: the int8 maximum falls, the norm maximum stays
    ids = np.array([first_removed, coarse8], np.int64)
    only_c8 = _index(d, 0, "auto", np.delete(x, [coarse8], 0))
    ref = _index(d, 0, "auto", np.delete(x, ids, 0))
    assert ix.remove_ids(ids) == 2
    b1 = ix.bounds()
    assert _bits(b1) == _bits(ref.bounds())
    assert b1["max_norm2"] == b0["max_norm2"] and b1["max_int8_err2"] <= only_c8.bounds()["max_int8_err2"]
    ref.close()
    only_c8.close()
    # (2) the largest-norm row leaves
    xs = np.delete(x, ids, 0)
    big2 = big - int((ids < big).sum())
    ids2 = np.array([big2], np.int64) if where == "moved part" else np.array([big2, 12000], np.int64)
    surv = np.delete(xs, ids2, 0)
    assert ix.remove_ids(ids2) == ids2.shape[0]
    b2 = ix.bounds()
    assert b2["max_norm2"] < 1.001 and b2["max_bf16_err2"] < b1["max_bf16_err2"] and b2["max_int8_err2"] < b1["max_int8_err2"]
    fresh = _index(d, 0, "auto", surv)
    _assert_same_as_fresh(ix, fresh, surv, 0, f"outliers removed ({where})", ks=(10,))
    ix.close()
    fresh.close()


def test_masked_search_uses_the_new_row_numbering():
    n, d, k = 40000, 768, 10
    x = _rows(n, d, 4)
    ids = _ids("random10", n, seed=8)
    surv = np.delete(x, ids, 0)
    ix = _index(d, 0, "auto", x)
    assert ix.remove_ids(ids) == ids.shape[0]
    fresh = _index(d, 0, "auto", surv)
    allow = np.random.default_rng(2).random(surv.shape[0]) < 0.3
    sub = np.flatnonzero(allow)
    q = _rows(16, d, 41)
    o = ko.FlatIndexOracle(d, 0)
    o.add(surv[sub])
    Dr, Ir = o.search(q, k)
    for nq in (1, 16):
        D, I = ix.search(q[:nq], k, allow=allow)
        Df, If = fresh.search(q[:nq], k, allow=allow)
        assert np.array_equal(I, If) and np.array_equal(D, Df) and allow[I].all()
        assert_topk_matches(D, I, Dr[:nq], sub[Ir[:nq]], o.rescore64(q[:nq], Ir[:nq]), f"masked after removal nq={nq}")
    with pytest.raises(ValueError):
        ix.search(q[:1], k, allow=np.ones(n, bool))                  # the old length no longer fits
    ix.close()
    fresh.close()


def test_add_after_remove_and_second_remove():
    n, d = 60000, 768
    x = _rows(n, d, 6)
    more = _rows(20000, d, 60)
    ids = _ids("block", n)
    ix = _index(d, 0, "auto", x)
    assert ix.remove_ids(ids) == ids.shape[0]
    ix.add(more)                                                     # appended behind the survivors
    cur = np.concatenate([np.delete(x, ids, 0), more])
    fresh = _index(d, 0, "auto", cur)
    _assert_same_as_fresh(ix, fresh, cur, 0, "add after remove", ks=(10,), queries=(1, 300))
    fresh.close()
    ids2 = _ids("random10", cur.shape[0], seed=12)
    assert ix.remove_ids(ids2) == ids2.shape[0]
    cur = np.delete(cur, ids2, 0)
    fresh = _index(d, 0, "auto", cur)
    _assert_same_as_fresh(ix, fresh, cur, 0, "second remove", ks=(10,), queries=(1, 300))
    ix.close()
    fresh.close()


def test_remove_right_behind_an_asynchronous_add_and_a_search_on_a_third_stream():
    """add_dev on a side stream, remove_ids at once, search_dev on a third stream: no synchronisation by the caller;
    the library orders the three by its events."""
    import torch

    n, d, k, nq = 400000, 768, 10, 16
    x = _rows(n, d, 14)
    ids = _ids("random10", n, seed=15)
    surv = np.delete(x, ids, 0)
    side, third = torch.cuda.Stream(), torch.cuda.Stream()
    xd = torch.from_numpy(x).cuda()
    q = _rows(nq, d, 16)
    qd = torch.from_numpy(q).cuda()
    Dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    Id = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix = _index(d, 0, "auto")
    ix.reserve(n)
    ix.add_dev(xd.data_ptr(), n, stream=side.cuda_stream)
    assert ix.remove_ids(ids) == ids.shape[0]
    ix.search_dev(qd.data_ptr(), nq, k, Dd.data_ptr(), Id.data_ptr(), third.cuda_stream)
    torch.cuda.synchronize()
    fresh = _index(d, 0, "auto", surv)
    Df, If = fresh.search(q, k)
    assert np.array_equal(Id.cpu().numpy(), If) and np.array_equal(Dd.cpu().numpy(), Df)
    _assert_same_as_fresh(ix, fresh, surv, 0, "behind an asynchronous add", ks=(10,), queries=(16,), oracle=False)
    ix.close()
    fresh.close()


def test_2m_device_generated_rows():
    from claude_semantic_search_amd.flat_index import IndexFlatIP

    n, d, seed = 2_000_000, 768, 21
    ix = IndexFlatIP(d)
    ix.reserve(n)
    ix.add_synthetic(n, seed=seed, first_row=0, normalize=True)
    keep = np.random.default_rng(22).random(n) >= 0.25
    assert ix.remove_ids(~keep) == int((~keep).sum())
    m = int(keep.sum())
    assert ix.ntotal == m
    old_of_new = np.flatnonzero(keep)
    sample = np.unique(np.concatenate([[0, 1, m - 2, m - 1], np.random.default_rng(23).integers(0, m, 200)]))
    for new in sample.tolist():
        want = ko.normalize_rows(ko.synth_rows(1, d, seed, first_row=int(old_of_new[new])))
        got = ix.reconstruct_n(new, 1)
        assert np.allclose(got, want, atol=1e-6, rtol=0), f"row {new} is not old row {old_of_new[new]}"
    fresh = IndexFlatIP(d)
    fresh.reserve(m)
    for r0 in range(0, m, 1 << 18):
        fresh.add(ix.reconstruct_n(r0, min(1 << 18, m - r0)))
    assert _bits(ix.bounds()) == _bits(fresh.bounds()) and ix.shadow_info() == fresh.shadow_info()
    q = _rows(300, d, 24)
    D, I = ix.search(q, 10)
    Df, If = fresh.search(q, 10)
    assert np.array_equal(I, If) and np.array_equal(D, Df)
    want = ko.normalize_rows(ko.synth_rows(1, d, seed, first_row=int(old_of_new[m // 2])))
    d1, i1 = ix.search(want, 1)
    assert i1[0, 0] == m // 2 and abs(d1[0, 0] - 1.0) < 1e-5
    ix.close()
    fresh.close()


def test_storage_compacts_without_a_second_copy_of_the_index(tmp_path):
    """HybridStorage.optimize() on the real index.  Margin: the free HBM read after optimize() may be lower than before
    it by at most 0.25 of one index footprint (fp32 + bf16 + int8 rows of all n rows); the in-place path allocates
    at most 64 MiB of bounce rows + 4 MiB of keep bits (0.04 footprints here), while a second index over the live half
    of the rows would hold 0.5 footprints."""
    from claude_semantic_search_amd import _native as nat
    from claude_semantic_search_amd.chunk import Chunk
    from claude_semantic_search_amd.storage import HybridStorage, StorageConfig

    n, d = 300_000, 768
    x = _rows(n, d, 31)
    s = HybridStorage(StorageConfig(data_dir=str(tmp_path), embedding_dim=d, auto_save=False))
    s.initialize()
    s.add_chunks([Chunk(f"c{i}", "t", {"session_id": f"s{i % 2}", "project_name": "p"}, x[i]) for i in range(n)])
    stored = s.faiss_index.reconstruct_n(0, n)
    index_before = s.faiss_index
    assert s.delete_chunks_by_session("s1") == n // 2 and s.faiss_index.ntotal == n
    footprint = n * (d * 4 + d * 2 + d + 8)
    free_before = nat.device_info(0)["hbm_free_bytes"]
    s.optimize()
    free_after = nat.device_info(0)["hbm_free_bytes"]
    print(f"free HBM before {free_before} after {free_after} (footprint {footprint})")
    assert s.faiss_index is index_before and s.faiss_index.ntotal == n // 2 and s.total_chunks == n // 2
    assert free_before - free_after <= 0.25 * footprint
    assert np.array_equal(s.faiss_index.reconstruct_n(0, n // 2), stored[0::2])
    for i in (0, 2, n - 2):
        hit = s.search(stored[i])[0]
        assert hit.chunk_id == f"c{i}" and abs(hit.similarity - 1.0) < 1e-5
    s.close()


def _stored_terms(lists):
    """``get_terms`` of rows that were given ``lists``, restated: per row the distinct terms ascending, their counts
    saturated at 255, and the number of tokens given."""
    uniq = [np.unique(np.asarray(r, np.int64), return_counts=True) for r in lists]
    off = np.concatenate([[0], np.cumsum([u.shape[0] for u, _ in uniq])]).astype(np.int64)
    terms = np.concatenate([u for u, _ in uniq] + [np.zeros(0, np.int64)]).astype(np.uint32)
    tfs = np.minimum(np.concatenate([c for _, c in uniq] + [np.zeros(0, np.int64)]), 255).astype(np.uint8)
    return off, terms, tfs, np.array([len(r) for r in lists], np.uint32)


def _assert_columns(ix, labels, priors, lists, what):
    """labels, priors and term lists of EVERY row of ``ix`` against their numpy restatement: ints equal, float bits
    equal, the defaults (-1, 0.0, the empty list) on rows that were never given a value."""
    assert ix.ntotal == labels.shape[0] == priors.shape[0] == len(lists), what
    got_l, got_p = ix.get_groups(), ix.get_priors()
    assert got_l.dtype == np.int32 and np.array_equal(got_l, labels), f"{what}: labels differ"
    assert got_p.dtype == np.float32 and np.array_equal(got_p.view(np.uint32), priors.view(np.uint32)), f"{what}: priors differ"
    for got, want, name in zip(ix.get_terms(), _stored_terms(lists), ("offsets", "terms", "tfs", "dl")):
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{what}: term list {name} differ"


@pytest.mark.parametrize("metric", [0, 1])
def test_labels_priors_and_terms_follow_the_rows_together(metric):
    """Labels AND priors (and term lists) on one index: the two columns share their life -- allocation at the default,
    capacity growth, the default of appended rows, compaction through the same keep-bit workspaces, reset -- so every
    step is checked against a numpy restatement of all three, and the searches that read the columns after the
    removal against an index freshly built from the kept rows, labels and priors (bit for bit)."""
    d, step = 64, 700
    rng = np.random.default_rng(100 + metric)
    x = _rows(6 * step + 200, d, 17)
    ix = _index(d, metric, "auto")
    labels, priors, lists = np.zeros(0, np.int32), np.zeros(0, np.float32), []

    def add(m, what):
        nonlocal labels, priors, lists
        n0 = ix.ntotal
        ix.add(x[n0:n0 + m])
        labels = np.concatenate([labels, np.full(m, -1, np.int32)])
        priors = np.concatenate([priors, np.zeros(m, np.float32)])
        lists = lists + [[] for _ in range(m)]
        _assert_columns(ix, labels, priors, lists, what)

    _assert_columns(ix, labels, priors, lists, "empty index")
    for i in range(3):                                               # 1024 -> 1536 -> 2304 rows of capacity
        add(step, f"add {i} (no column yet)")
    # 1. labels on [100, 2100), a few negative (stored as -1)
    given = rng.integers(0, 40, 2000).astype(np.int32)
    given[rng.integers(0, 2000, 25)] = -7
    ix.set_groups(given, row0=100)
    labels[100:2100] = np.maximum(given, -1)
    _assert_columns(ix, labels, priors, lists, "labels set")
    add(step, "growth with labels only")                             # 2304 -> 3456
    # 2. priors on [500, 2500)
    given_p = rng.normal(0.0, 0.2, 2000).astype(np.float32)
    ix.set_priors(given_p, row0=500)
    priors[500:2500] = given_p
    _assert_columns(ix, labels, priors, lists, "priors set")
    # 3. term lists on the leading 1500 rows (repeats, empty rows, one term more than 255 times)
    given_t = [rng.integers(0, 300, int(rng.integers(0, 12))).tolist() for _ in range(1500)]
    given_t[7] = [5] * 300 + [2]
    ix.set_terms(given_t)
    lists[:1500] = given_t
    _assert_columns(ix, labels, priors, lists, "terms set")
    # 4. growth again, with every column set: 3456 -> 5184
    add(step, "growth with all columns (fits)")
    add(step, "growth with all columns")
    n = ix.ntotal
    assert n == 6 * step
    # 5. about 10 % of the rows leave: row 0, a row of the last 32-row word, a run longer than 32 rows
    dead = rng.random(n) < 0.10
    dead[[0, n - 3]] = True
    dead[1000:1045] = True
    keep = np.flatnonzero(~dead)
    assert ix.remove_ids(np.flatnonzero(dead)) == int(dead.sum())
    labels, priors, lists = labels[keep], priors[keep], [lists[i] for i in keep]
    _assert_columns(ix, labels, priors, lists, "removed")
    fresh = _index(d, metric, "auto", x[keep])
    fresh.set_groups(labels)
    fresh.set_priors(priors)
    q = _rows(3, d, 18)
    for got, want, name in zip(ix.search_grouped(q, 10), fresh.search_grouped(q, 10), "DIG"):
        assert np.array_equal(got.view(np.uint32) if name == "D" else got, want.view(np.uint32) if name == "D" else want), \
            f"search_grouped {name} differs from a freshly built index"
    for got, want, name in zip(ix.search_prior(q, 10, 0.25), fresh.search_prior(q, 10, 0.25), "DIS"):
        assert np.array_equal(got.view(np.uint32) if name != "I" else got, want.view(np.uint32) if name != "I" else want), \
            f"search_prior {name} differs from a freshly built index"
    fresh.close()
    # 6. rows appended behind the survivors start at the defaults (the slots held other rows' values)
    add(100, "add after remove")
    # 7. reset forgets every column; an index that never set one answers the defaults as well
    ix.reset()
    labels, priors, lists = np.zeros(0, np.int32), np.zeros(0, np.float32), []
    add(step, "add after reset")
    ix.close()
