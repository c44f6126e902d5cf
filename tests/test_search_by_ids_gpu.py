"""GPU: ``IndexFlat.search_by_ids`` (``css_index_search_rows``) -- stored rows as queries, the anchor dropped on the
device.

The oracle of the equivalence tests is the plain search of the SAME index, which this feature does not touch:

    expected = index.search(index.reconstruct_n()[anchors - id_base], k + 1)

post-processed in numpy by the rule of ``k_drop_self`` (the anchor's entry goes where it is present, the last entry
otherwise).  Both sides run the same kernels on the same query bits, so ``exact_fp32`` results must be bit-identical;
the candidate path (``coarse``) is held to the suite's usual comparison (``knn_checks.assert_topk_matches``).

2999 rows: no multiple of any tile.  nq 1 / 3 / 5 / 17 / 33 are the query-count paths named in ``css_hip.h`` (one query
cascade, 3..4, 5..16, batches of more than 16, more than 32); k 31 / 32 and 127 / 128 put ``k + 1`` on either side of
the 32 / 33 and 128 / 129 (second pass) boundaries."""
import numpy as np
import pytest

from oracle import knn_oracle as ko
from knn_checks import assert_topk_matches

pytestmark = pytest.mark.gpu

N = 2999
NQS = (1, 3, 5, 17, 33)
KS = (1, 10, 31, 32, 127, 128)
FLT_MAX = np.finfo(np.float32).max


def _index(d, metric, x, shadow=None, id_base=0):
    from claude_semantic_search_amd.flat_index import IndexFlat

    ix = IndexFlat(d, metric)
    ix.set_shadow(shadow)
    if id_base:
        ix.set_id_base(id_base)
    if x.shape[0]:
        ix.add(x)
    return ix


def _rows(n, d, seed, metric=0):
    x = ko.synth_rows(n, d, seed)
    return ko.normalize_rows(x) if metric == 0 else x      # inner product: unit rows; L2: raw rows


def _drop(D, I, anchors):
    """numpy statement of the rule: [nq, k + 1] -> [nq, k]."""
    nq, kk = I.shape
    out_d, out_i = np.empty((nq, kk - 1), np.float32), np.empty((nq, kk - 1), np.int64)
    for j in range(nq):
        hit = np.flatnonzero(I[j] == anchors[j])
        p = int(hit[0]) if hit.size else kk - 1
        out_d[j], out_i[j] = np.delete(D[j], p), np.delete(I[j], p)
    return out_d, out_i


def _expected(ix, anchors, k, id_base=0, allow=None):
    rows = ix.reconstruct_n()[np.asarray(anchors) - id_base]
    D, I = ix.search(rows, k + 1, allow=allow)
    return _drop(D, I, anchors)


def _anchors(nq, seed, n=N):
    return np.random.default_rng(seed).choice(n, size=nq, replace=False).astype(np.int64)


def _d64(x, metric, anchors, I):
    ref = ko.FlatIndexOracle(x.shape[1], metric)
    ref.add(x)
    return ref.rescore64(x[anchors], np.where(I < 0, 0, I))


@pytest.mark.parametrize("d", [64, 100, 384, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_exact_fp32_is_bit_identical_to_the_plain_search(metric, d):
    x = _rows(N, d, 11 + d, metric)
    ix = _index(d, metric, x)
    ix.set_search_mode("exact_fp32")
    for nq in NQS:
        anchors = _anchors(nq, nq)
        for k in KS:
            D, I = ix.search_by_ids(anchors, k)
            De, Ie = _expected(ix, anchors, k)
            what = f"metric={metric} d={d} nq={nq} k={k}"
            assert np.array_equal(I, Ie), what
            assert np.array_equal(D.view(np.uint32), De.view(np.uint32)), what
            assert not (I == anchors[:, None]).any(), what
    ix.close()


@pytest.mark.parametrize("shadow", [False, True, "int8"], ids=["noshadow", "bf16", "int8"])
@pytest.mark.parametrize("d", [64, 100, 384, 768])
@pytest.mark.parametrize("metric", [0, 1])
def test_coarse_mode_under_every_shadow_policy(metric, d, shadow):
    x = _rows(N, d, 23 + d, metric)
    ix = _index(d, metric, x, shadow=shadow)
    ix.set_search_mode("coarse")
    for nq in NQS:
        anchors = _anchors(nq, 100 + nq)
        for k in KS:
            D, I = ix.search_by_ids(anchors, k)
            De, Ie = _expected(ix, anchors, k)
            what = f"coarse shadow={shadow} metric={metric} d={d} nq={nq} k={k}"
            assert_topk_matches(D, I, De, Ie, _d64(x, metric, anchors, Ie), what)
            assert not (I == anchors[:, None]).any(), what
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "auto"])
@pytest.mark.parametrize("metric", [0, 1])
def test_without_exclude_self_it_is_the_search_of_those_rows(metric, mode):
    x = _rows(N, 384, 5, metric)
    ix = _index(384, metric, x)
    ix.set_search_mode(mode)
    for nq, k in ((1, 10), (5, 1), (17, 32), (33, 128), (3, 129)):
        anchors = _anchors(nq, 7 * nq)
        D, I = ix.search_by_ids(anchors, k, exclude_self=False)
        De, Ie = ix.search(x[anchors], k)
        if mode == "exact_fp32":
            assert np.array_equal(I, Ie) and np.array_equal(D.view(np.uint32), De.view(np.uint32))
        else:
            assert_topk_matches(D, I, De, Ie, _d64(x, metric, anchors, Ie), f"metric={metric} nq={nq} k={k}")
        assert (I[:, 0] == anchors).all()            # distinct rows: every anchor is its own best match
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "auto", "coarse"])
@pytest.mark.parametrize("metric", [0, 1])
def test_duplicates_of_the_anchor_are_ordinary_results(metric, mode):
    x = _rows(500, 64, 9, metric)
    x[10] = x[250]
    x[400] = x[250]
    ix = _index(64, metric, x)
    ix.set_search_mode(mode)
    Ds, Is = ix.search_by_ids([250], 3, exclude_self=False)
    assert Is[0].tolist() == [10, 250, 400] and Ds[0, 0] == Ds[0, 1] == Ds[0, 2]      # ties: lower id first
    D, I = ix.search_by_ids([250], 5)
    assert I[0, :2].tolist() == [10, 400] and 250 not in I[0].tolist()
    assert D[0, 0] == Ds[0, 1] and D[0, 1] == Ds[0, 1]                                 # the self score
    # seen from a copy, the anchor of before is an ordinary result too
    D2, I2 = ix.search_by_ids([10, 400], 2)
    assert I2.tolist() == [[250, 400], [10, 250]]
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "auto"])
def test_unnormalised_inner_product_where_a_row_is_not_its_own_best_match(mode):
    n, d, k = N, 100, 10
    x = ko.normalize_rows(ko.synth_rows(n, d, 31))
    norms = np.geomspace(0.1, 10.0, n).astype(np.float32)
    np.random.default_rng(3).shuffle(norms)
    x = np.ascontiguousarray(x * norms[:, None])
    ix = _index(d, 0, x)
    ix.set_search_mode(mode)
    anchors = np.argsort(norms)[:5].astype(np.int64)                  # the five shortest rows
    _, Iself = ix.search_by_ids(anchors, k + 1, exclude_self=False)
    assert not (Iself == anchors[:, None]).any()                      # not among their own k + 1 best
    D, I = ix.search_by_ids(anchors, k)
    s = x[anchors].astype(np.float64) @ x.astype(np.float64).T
    s[np.arange(5), anchors] = -np.inf
    Ir = np.stack([np.lexsort((np.arange(n), -s[j]))[:k] for j in range(5)]).astype(np.int64)
    D64 = np.take_along_axis(s, Ir, axis=1)
    assert_topk_matches(D, I, D64.astype(np.float32), Ir, D64, f"raw inner product [{mode}]")
    ix.close()


@pytest.mark.parametrize("mode", ["exact_fp32", "auto"])
@pytest.mark.parametrize("metric", [0, 1])
def test_masks(metric, mode):
    x = _rows(N, 384, 41, metric)
    ix = _index(384, metric, x)
    ix.set_search_mode(mode)
    anchors = _anchors(5, 8)
    allow = np.random.default_rng(2).random(N) < 0.5
    for anchor_allowed in (True, False):
        allow[anchors] = anchor_allowed
        for k in (10, 128):
            D, I = ix.search_by_ids(anchors, k, allow=allow)
            De, Ie = _expected(ix, anchors, k, allow=allow)
            if mode == "exact_fp32":
                assert np.array_equal(I, Ie) and np.array_equal(D.view(np.uint32), De.view(np.uint32))
            else:
                assert_topk_matches(D, I, De, Ie, _d64(x, metric, anchors, Ie), f"masked, anchor allowed={anchor_allowed}")
            assert allow[I].all() and not (I == anchors[:, None]).any()
    # fewer than k allowed rows: the rest of the row is padding
    few = np.zeros(N, bool)
    few[[7, 1500, int(anchors[0])]] = True
    D, I = ix.search_by_ids(anchors[:1], 10, allow=few)
    assert sorted(I[0, :2].tolist()) == [7, 1500] and (I[0, 2:] == -1).all()
    assert (D[0, 2:] == (-FLT_MAX if metric == 0 else FLT_MAX)).all()
    ix.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_an_index_of_one_row_gives_an_all_padded_result(metric):
    ix = _index(64, metric, _rows(1, 64, 1, metric))
    D, I = ix.search_by_ids([0, 0], 4)
    assert (I == -1).all() and (D == (-FLT_MAX if metric == 0 else FLT_MAX)).all()
    D, I = ix.search_by_ids([0], 1, exclude_self=False)
    assert I.tolist() == [[0]]
    ix.close()


def test_id_base_and_repeated_anchors():
    base = 10**9
    x = _rows(N, 100, 51)
    ix = _index(100, 0, x, id_base=base)
    ix.set_search_mode("exact_fp32")
    anchors = base + np.array([5, 5, 2998, 7, 5, 0], np.int64)
    for k in (10, 128):
        D, I = ix.search_by_ids(anchors, k)
        De, Ie = _expected(ix, anchors, k, id_base=base)
        assert np.array_equal(I, Ie) and np.array_equal(D.view(np.uint32), De.view(np.uint32))
        assert I.min() >= base and not (I == anchors[:, None]).any()
        assert np.array_equal(I[0], I[1]) and np.array_equal(I[0], I[4]) and np.array_equal(D[0], D[4])
    ix.close()


def test_after_remove_ids_and_capacity_growth_it_equals_a_fresh_index():
    d = 384
    x = _rows(9000, d, 61)
    ix = _index(d, 0, x[:1000])
    gone = np.arange(3, 1000, 7)
    assert ix.remove_ids(gone) == gone.size
    ix.add(x[1000:])                                                   # grows the capacity several times over
    surv = np.delete(x, gone, axis=0)
    fresh = _index(d, 0, surv)
    assert ix.ntotal == fresh.ntotal == surv.shape[0]
    anchors = np.array([0, 2, 3, 856, 857, surv.shape[0] - 1, 4321], np.int64)
    for nq, k in ((1, 10), (7, 10), (7, 128)):
        D, I = ix.search_by_ids(anchors[:nq], k)
        Df, If = fresh.search_by_ids(anchors[:nq], k)
        assert np.array_equal(I, If) and np.array_equal(D.view(np.uint32), Df.view(np.uint32))
        De, Ie = _expected(fresh, anchors[:nq], k)
        assert_topk_matches(D, I, De, Ie, _d64(surv, 0, anchors[:nq], Ie), f"after remove_ids, nq={nq} k={k}")
    ix.close()
    fresh.close()


def _dev_search(ix, ids_t, k, exclude_self=True, stream=None):
    import torch

    nq = ids_t.shape[0]
    D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    I = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        ix.search_by_ids_dev(ids_t.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), stream=st.cuda_stream,
                             exclude_self=exclude_self)
    st.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def test_rows_added_on_another_stream_right_before_the_device_call_are_found():
    import torch

    from claude_semantic_search_amd.flat_index import IndexFlatIP

    d, n0, n1 = 256, 2999, 150_000
    ix = IndexFlatIP(d)
    ix.add(_rows(n0, d, 71))
    ix.reserve(n0 + n1)
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    ids = torch.tensor([n0, n0 + n1 - 1, n0 + 77_777, 5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        fresh = torch.nn.functional.normalize(torch.randn((n1, d), device="cuda"), dim=1).contiguous()
        ix.add_dev(fresh.data_ptr(), n1, stream=side.cuda_stream)      # only enqueued
    D, I = _dev_search(ix, ids, 1, exclude_self=False, stream=other)   # no caller-side synchronisation in between
    assert I[:, 0].tolist() == ids.tolist() and np.all(np.abs(D - 1.0) < 1e-5)
    D, I = _dev_search(ix, ids, 10, stream=other)
    assert not (I == ids.cpu().numpy()[:, None]).any() and (I >= 0).all()
    De, Ie = _expected(ix, ids.cpu().numpy(), 10)
    x_all = ix.reconstruct_n()
    assert_topk_matches(D, I, De, Ie, _d64(x_all, 0, ids.cpu().numpy(), Ie), "behind add_dev on another stream")
    del fresh
    ix.close()


def test_host_form_errors():
    from claude_semantic_search_amd import _native as nat
    from claude_semantic_search_amd.flat_index import MAX_K

    x = _rows(300, 64, 81)
    ix = _index(64, 0, x, id_base=1000)
    for bad in (999, 1300, -1, 0):
        with pytest.raises(nat.CssError, match=str(bad)) as e:
            ix.search_by_ids([1000, bad, 1001], 5)
        assert e.value.code == nat.CSS_ERR_INVALID
    with pytest.raises(ValueError):
        ix.search_by_ids([1000], MAX_K)                                # exclude_self searches for k + 1
    ix.search_by_ids([1000], MAX_K, exclude_self=False)
    ix.search_by_ids([1000], MAX_K - 1)
    D = np.empty((1, MAX_K), np.float32)
    I = np.empty((1, MAX_K), np.int64)
    one = np.array([1000], np.int64)
    rc = nat.lib().css_index_search_rows(ix._handle(), one.ctypes.data, 1, MAX_K, 1, None, D.ctypes.data, I.ctypes.data)
    assert rc == nat.CSS_ERR_INVALID
    for ids in ([1000.0], ["a"], [True], np.array([1000.5])):
        with pytest.raises(ValueError):
            ix.search_by_ids(ids, 5)
    D, I = ix.search_by_ids([], 7)
    assert D.shape == (0, 7) and I.shape == (0, 7) and D.dtype == np.float32 and I.dtype == np.int64
    assert nat.lib().css_index_search_rows(ix._handle(), None, 0, 5, 1, None, None, None) == nat.CSS_OK
    ix.close()
    empty = _index(64, 0, np.zeros((0, 64), np.float32))
    with pytest.raises(nat.CssError):
        empty.search_by_ids([0], 1)
    empty.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_device_form_pads_queries_with_invalid_ids_and_leaves_the_others_alone(metric):
    import torch

    base = 1000
    x = _rows(N, 100, 91, metric)
    ix = _index(100, metric, x, id_base=base)
    pad = -FLT_MAX if metric == 0 else FLT_MAX
    ids = np.array([base + 4, -5, base + 2998, base + N, base, base - 1, base + 17], np.int64)
    valid = (ids >= base) & (ids < base + N)
    stand_in = np.where(valid, ids, base + 1)                          # the same query count for the host form: the same kernels
    for mode in ("exact_fp32", "auto"):
        ix.set_search_mode(mode)
        for k, excl in ((10, True), (128, True), (10, False)):
            D, I = _dev_search(ix, torch.from_numpy(ids).cuda(), k, exclude_self=excl)
            assert (I[~valid] == -1).all() and (D[~valid] == pad).all()
            Dh, Ih = ix.search_by_ids(stand_in, k, exclude_self=excl)
            if mode == "exact_fp32":
                assert np.array_equal(I[valid], Ih[valid]) and np.array_equal(D[valid].view(np.uint32), Dh[valid].view(np.uint32))
            else:
                assert_topk_matches(D[valid], I[valid], Dh[valid], Ih[valid], _d64(x, metric, ids[valid] - base, Ih[valid] - base),
                                    f"device form, metric={metric} k={k} exclude_self={excl}")
    ix.close()
    empty = _index(100, metric, np.zeros((0, 100), np.float32))
    D, I = _dev_search(empty, torch.tensor([0, 1], dtype=torch.int64, device="cuda"), 3)
    assert (I == -1).all() and (D == pad).all()
    empty.search_by_ids_dev(0, 0, 3, 0, 0)                             # nq = 0: a no-op, nothing is dereferenced
    empty.close()
