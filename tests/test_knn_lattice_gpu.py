"""Exact-tie tests of the core search, ``search_by_ids``, ``range_search`` and the shard merges on lattice rows.

On the rows of tests/lattice_cases.py every score is exact in fp32 whatever the summation order, the operand format
(fp32, bf16, split operands) or the form of the squared distance, so every search mode, shadow policy and query-count
class must return the SAME BITS: ``D`` equal to the float64 truth cast to float32 and ``I`` equal to
``np.lexsort((id, -score))`` -- best first, ties to the lower id, the order include/css_hip.h promises.  There is no
tolerance, no tie window and no excluded slot (``lattice_cases.assert_exact``).  Ties straddle rank k, the pass
boundaries at 128 and 256 and the shard boundaries in most queries (tests/test_knn_lattice_host.py counts them).

The int8 rows of family T are exact up to their fp32 scale (amax = 1 gives bytes of +-127), so the measured error of the
coarse copies is ~0 and the band of the candidate path is its floor term alone, 2^-11 * ||q|| * max||x|| ~ 0.25 against
integer scores: the band holds precisely the exact ties of the k-th best.  Family E has exact bf16 rows but inexact int8
rows (0.125 * 127 is no integer): an ordinary band with exact final scores.

tests/test_knn_lattice_forced_gpu.py runs this file again under the switches that select the paths a small index does
not reach by itself."""
import ctypes

import numpy as np
import pytest

import lattice_cases as lc

pytestmark = pytest.mark.gpu

SHAPES = {"T20k": ("T", 20000, 768), "T6k": ("T", 6000, 200), "T4k": ("T", 4000, 64), "E20k": ("E", 20000, 768)}
# (metric, shadow policy): the inner product on every policy, L2 on the automatic one and without shadow rows
POLICIES = [(0, None), (0, "int8"), (0, False), (1, None), (1, False)]
NQS = (1, 3, 4, 12, 16, 17, 33, 40, 300)
KS = (1, 10, 32, 33, 64, 100, 128)


def _pid(v):
    return {None: "auto", "int8": "int8", False: "none"}.get(v, str(v)) if not isinstance(v, tuple) else \
        ("ip" if v[0] == 0 else "l2") + "-" + _pid(v[1])


class Cases:
    """Rows, queries, float64 scores and the sorted truth per (shape, metric), one index per (shape, metric, policy):
    each built once for the module."""

    def __init__(self):
        self.data, self.truth, self.index = {}, {}, {}

    def rows(self, shape):
        if shape not in self.data:
            self.data[shape] = lc.case(*SHAPES[shape])
        return self.data[shape]

    def scores(self, shape, metric):
        """``(S float64 [300, n], D, I)``: the scores and the whole truth list to the largest k a test asks for."""
        if (shape, metric) not in self.truth:
            x, q = self.rows(shape)
            S = lc.scores64(x, q, metric)
            self.truth[shape, metric] = (S,) + lc.topk_of_scores(S, 2048 if shape == "T6k" else 300, metric)
        return self.truth[shape, metric]

    def top(self, shape, metric, nq, k):
        _, D, I = self.scores(shape, metric)
        assert k <= D.shape[1]
        return D[:nq, :k], I[:nq, :k]            # (a total order: every prefix of the list is the truth of its k)

    def ix(self, shape, metric, policy):
        from claude_semantic_search_amd.flat_index import IndexFlat

        key = (shape, metric, policy)
        if key not in self.index:
            x, _ = self.rows(shape)
            ix = IndexFlat(x.shape[1], metric)
            ix.set_shadow(policy)
            ix.add(x)
            self.index[key] = ix
        ix = self.index[key]
        ix.set_search_mode("auto")
        return ix

    def close(self):
        for ix in self.index.values():
            ix.close()


@pytest.fixture(scope="module")
def cases():
    c = Cases()
    yield c
    c.close()


# ---- plain search -----------------------------------------------------------------------------------------------------
# (the split-operand scan is the path of shadow-less indexes: only they run it)
PLAIN = [(shape, mp, mode) for shape in SHAPES for mp in POLICIES for mode in ("exact_fp32", "coarse", "auto", "split")
         if mode != "split" or mp[1] is False]


@pytest.mark.parametrize("shape,mp,mode", PLAIN, ids=[f"{s}-{_pid(mp)}-{m}" for s, mp, m in PLAIN])
def test_plain_search_returns_the_truth_bit_for_bit(cases, shape, mp, mode):
    metric, policy = mp
    x, q = cases.rows(shape)
    ix = cases.ix(shape, metric, policy)
    ix.set_search_mode(mode)
    if mode == "split":
        grid = [(nq, k) for nq in (17, 33, 40, 300) for k in KS]
    elif policy is None:
        grid = [(nq, k) for nq in NQS for k in KS]                       # every query-count class x every k
    else:
        grid = [(nq, k) for nq in (1, 3, 12, 40, 300) for k in (10, 64, 128)]
    for nq, k in grid:
        D, I = ix.search(q[:nq], k)
        lc.assert_exact(D, I, *cases.top(shape, metric, nq, k), f"{shape} {_pid(mp)} [{mode}] nq={nq} k={k}")


# ---- k beyond one pass: the order inside the list, across the boundaries at 128 and 256 ---------------------------------
@pytest.mark.parametrize("mp", POLICIES, ids=_pid)
@pytest.mark.parametrize("shape,k", [("T20k", 129), ("T20k", 300), ("E20k", 300), ("T4k", 129), ("T4k", 300),
                                     ("T6k", 129), ("T6k", 300), ("T6k", 2048)])
def test_k_beyond_one_pass_keeps_the_total_order(cases, shape, k, mp):
    metric, policy = mp
    _, q = cases.rows(shape)
    ix = cases.ix(shape, metric, policy)
    for mode in ("exact_fp32", "coarse", "auto"):
        ix.set_search_mode(mode)
        for nq in (1, 3):
            D, I = ix.search(q[:nq], k)
            lc.assert_exact(D, I, *cases.top(shape, metric, nq, k), f"{shape} {_pid(mp)} [{mode}] nq={nq} k={k}")


# ---- masks ------------------------------------------------------------------------------------------------------------
def _masks(n):
    _, _, blk = lc.planted(n)
    rng = np.random.default_rng(5)
    dense = rng.random(n) < 0.3
    sparse = np.zeros(n, dtype=bool)
    sparse[rng.choice(n, 7, replace=False)] = True                       # fewer allowed rows than k: pads appear
    part = np.ones(n, dtype=bool)
    part[blk + 3:blk + lc.COPIES:2] = False                              # only part of the block of copies
    return {"dense": dense, "sparse": sparse, "part": part}


@pytest.mark.parametrize("mp", POLICIES, ids=_pid)
@pytest.mark.parametrize("shape", ["T20k", "T4k"])
def test_masked_search_returns_the_truth_of_the_allowed_rows(cases, shape, mp):
    metric, policy = mp
    x, q = cases.rows(shape)
    S = cases.scores(shape, metric)[0]
    ix = cases.ix(shape, metric, policy)
    blk = lc.planted(x.shape[0])[2]
    qq = q[:40].copy()
    qq[0] = x[blk]                                                        # one query IS the copied row: 40 equal best scores
    S = S[:40].copy()
    S[0] = lc.scores64(x, qq[:1], metric)[0]
    for name, allow in _masks(x.shape[0]).items():
        truth = {k: lc.topk_of_scores(S, k, metric, allow=allow) for k in (10, 300)}
        for mode in ("exact_fp32", "coarse", "auto"):
            ix.set_search_mode(mode)
            for nq in (1, 40):
                for k in (10, 300):
                    D, I = ix.search(qq[:nq], k, allow=allow)
                    Dt, It = truth[k]
                    lc.assert_exact(D, I, Dt[:nq], It[:nq], f"{shape} {_pid(mp)} [{mode}] mask={name} nq={nq} k={k}")


# ---- growth and removal -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", [(0, None), (0, "int8"), (1, None)], ids=_pid)
def test_growth_in_three_adds_then_remove_every_third_row(cases, mp):
    from claude_semantic_search_amd.flat_index import IndexFlat

    metric, policy = mp
    x, q = cases.rows("T6k")
    n = x.shape[0]
    ix = IndexFlat(x.shape[1], metric)
    ix.set_shadow(policy)
    for lo, hi in ((0, 700), (700, 2900), (2900, n)):                    # no reserve: every add outgrows the allocation
        ix.add(x[lo:hi])
    for nq, k in ((3, 100), (40, 10)):
        D, I = ix.search(q[:nq], k)
        lc.assert_exact(D, I, *cases.top("T6k", metric, nq, k), f"grown {_pid(mp)} nq={nq} k={k}")
    gone = np.arange(0, n, 3)
    assert ix.remove_ids(gone) == gone.size
    keep = np.ones(n, dtype=bool)
    keep[gone] = False
    S = cases.scores("T6k", metric)[0][:40][:, keep]                     # the compacted rows: ids are their new positions
    for mode in ("exact_fp32", "coarse", "auto"):
        ix.set_search_mode(mode)
        for nq, k in ((3, 100), (40, 10), (2, 300)):
            D, I = ix.search(q[:nq], k)
            Dt, It = lc.topk_of_scores(S[:nq], k, metric)
            lc.assert_exact(D, I, Dt, It, f"after remove_ids {_pid(mp)} [{mode}] nq={nq} k={k}")
    ix.close()


# ---- device twin --------------------------------------------------------------------------------------------------------
def test_search_dev_with_a_device_bitmap_equals_the_host_call(cases):
    import torch

    from claude_semantic_search_amd.flat_index import pack_allow_bits

    x, q = cases.rows("T20k")
    n, nq, k = x.shape[0], 3, 300
    ix = cases.ix("T20k", 0, None)
    allow = _masks(n)["dense"]
    D, I = ix.search(q[:nq], k, allow=allow)
    qd = torch.from_numpy(q[:nq]).cuda()
    Dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    Id = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    bits = torch.from_numpy(pack_allow_bits(allow, n).view(np.int32)).cuda()
    ix.search_dev(qd.data_ptr(), nq, k, Dd.data_ptr(), Id.data_ptr(), torch.cuda.current_stream().cuda_stream,
                  allow_bits_ptr=bits.data_ptr())
    torch.cuda.synchronize()
    lc.assert_exact(Dd.cpu().numpy(), Id.cpu().numpy(), D, I, "search_dev against search")
    lc.assert_exact(D, I, *lc.topk_of_scores(cases.scores("T20k", 0)[0][:nq], k, 0, allow=allow), "search against the truth")


# ---- search_by_ids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", POLICIES, ids=_pid)
def test_search_by_ids_on_copies_the_zero_row_and_ordinary_rows(cases, mp):
    metric, policy = mp
    x, _ = cases.rows("T20k")
    n = x.shape[0]
    zero, src, blk = lc.planted(n)
    # a row of the block of copies, the all-zero row (inner product: EVERY score is 0, the list is the lowest ids), the
    # copied row itself, ordinary rows, one id twice
    anchors = np.array([blk + 5, zero, src, 17, n - 1, 17], dtype=np.int64)
    S = lc.scores64(x, x[anchors], metric)
    ix = cases.ix("T20k", metric, policy)
    hidden = np.ones(n, dtype=bool)
    hidden[anchors] = False                                              # a mask that does not allow the anchors
    hidden[blk + 1:blk + lc.COPIES:3] = False
    for mode in ("exact_fp32", "coarse", "auto"):
        ix.set_search_mode(mode)
        for k in (10, 129):
            for excl in (True, False):
                for allow in (None, hidden):
                    D, I = ix.search_by_ids(anchors, k, exclude_self=excl, allow=allow)
                    Dt, It = lc.topk_of_scores(S, k, metric, allow=allow, exclude=anchors if excl else None)
                    lc.assert_exact(D, I, Dt, It, f"search_by_ids {_pid(mp)} [{mode}] k={k} exclude_self={excl} "
                                                  f"mask={'no' if allow is None else 'yes'}")
        D, I = ix.search_by_ids(anchors[:1], 10)                         # one anchor: the few-query paths
        lc.assert_exact(D, I, *lc.topk_of_scores(S[:1], 10, metric, exclude=anchors[:1]), f"one anchor {_pid(mp)} [{mode}]")


# ---- range_search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", POLICIES, ids=_pid)
def test_range_search_at_attained_radii_is_strict_and_ordered(cases, mp):
    metric, policy = mp
    x, q = cases.rows("T20k")
    S, Dt, _ = cases.scores("T20k", metric)
    ix = cases.ix("T20k", metric, policy)
    # radii that ARE scores of query 0 (rows exactly there are no hits), one that nothing passes, one that everything does
    radii = [float(Dt[0, 9]), float(Dt[0, 199])]
    radii += [float(S.max() + 1), -np.inf] if metric == 0 else [-np.inf, 0.0, np.inf]
    assert (S[0] == radii[0]).any() and (S[0] == radii[1]).any()
    dense = _masks(x.shape[0])["dense"]
    for nq in (1, 3, 40):
        for r in radii:
            for allow in (None, dense):
                if np.isinf(r) and r > 0 and nq == 40 and allow is None:
                    continue                                              # (800 000 hits once, for the inner product, are enough)
                got = ix.range_search(q[:nq], r, allow=allow)
                what = f"range_search {_pid(mp)} nq={nq} radius={r} mask={'no' if allow is None else 'yes'}"
                lc.assert_exact_range(got, lc.range_of_scores(S[:nq], r, metric, allow=allow), what)


# ---- shards and merges against the truth ---------------------------------------------------------------------------------
BOUNDS = [0, 90, 1500, 20000]     # shard 0 has 90 rows: it pads inside its list from k = 128 on


@pytest.fixture(scope="module")
def shards(cases):
    from claude_semantic_search_amd.flat_index import IndexFlat

    x, _ = cases.rows("T20k")
    made = {}
    for metric in (0, 1):
        made[metric] = []
        for lo, hi in zip(BOUNDS[:-1], BOUNDS[1:]):
            s = IndexFlat(x.shape[1], metric)
            s.add(x[lo:hi])
            s.set_id_base(lo)
            made[metric].append(s)
    yield made
    for lst in made.values():
        for s in lst:
            s.close()


def _merge_dense(Dp, Ip, nq, k, metric, st):
    import torch

    from claude_semantic_search_amd import _native as nat

    Do = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    Io = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    nat.check(nat.lib().css_merge_topk_dev(ctypes.c_void_p(Dp.data_ptr()), ctypes.c_void_p(Ip.data_ptr()), Dp.shape[0], nq, k,
                                           metric, ctypes.c_void_p(Do.data_ptr()), ctypes.c_void_p(Io.data_ptr()), 0,
                                           ctypes.c_void_p(st)))
    torch.cuda.synchronize()
    return Do.cpu().numpy(), Io.cpu().numpy()


def _merge_packed(recv, record, nq, k, metric, st):
    import torch

    from claude_semantic_search_amd import _native as nat

    Do = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    Io = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    nat.check(nat.lib().css_merge_topk_packed_dev(ctypes.c_void_p(recv.data_ptr()), recv.shape[0], record, nq, k, metric,
                                                  ctypes.c_void_p(Do.data_ptr()), ctypes.c_void_p(Io.data_ptr()), 0,
                                                  ctypes.c_void_p(st)))
    torch.cuda.synchronize()
    return Do.cpu().numpy(), Io.cpu().numpy()


@pytest.mark.parametrize("k", [10, 128, 129, 700])
@pytest.mark.parametrize("metric", [0, 1])
def test_shard_lists_merge_to_the_truth_of_the_whole_index(cases, shards, metric, k):
    import torch

    from claude_semantic_search_amd.sharded import packed_layout

    x, q = cases.rows("T20k")
    S = cases.scores("T20k", metric)[0]
    G = len(BOUNDS) - 1
    st = torch.cuda.current_stream().cuda_stream
    for nq in (3, 40):
        Dt, It = lc.topk_of_scores(S[:nq], k, metric)
        qd = torch.from_numpy(q[:nq]).cuda()
        Dp = torch.empty((G, nq, k), dtype=torch.float32, device="cuda")
        Ip = torch.empty((G, nq, k), dtype=torch.int64, device="cuda")
        ib, db, record = packed_layout(nq, k)
        recv = torch.zeros((G, record), dtype=torch.uint8, device="cuda")
        for g, s in enumerate(shards[metric]):
            s.search_dev(qd.data_ptr(), nq, k, Dp[g].data_ptr(), Ip[g].data_ptr(), st)
            s.search_dev(qd.data_ptr(), nq, k, recv[g, ib:db].view(torch.float32).data_ptr(),
                         recv[g, :ib].view(torch.int64).data_ptr(), st)
        torch.cuda.synchronize()
        # every shard's own list is the truth of its rows (with its id base), pads at the tail
        for g, (lo, hi) in enumerate(zip(BOUNDS[:-1], BOUNDS[1:])):
            Dg, Ig = lc.topk_of_scores(S[:nq, lo:hi], k, metric, id_base=lo)
            lc.assert_exact(Dp[g].cpu().numpy(), Ip[g].cpu().numpy(), Dg, Ig, f"shard {g} metric={metric} nq={nq} k={k}")
        lc.assert_exact(*_merge_dense(Dp, Ip, nq, k, metric, st), Dt, It, f"dense merge metric={metric} nq={nq} k={k}")
        lc.assert_exact(*_merge_packed(recv, record, nq, k, metric, st), Dt, It, f"packed merge metric={metric} nq={nq} k={k}")


# ---- the merge kernels alone, on made-up part lists -------------------------------------------------------------------------
def _made_up_parts(G, k, nq, metric, seed):
    """``(Dp [G, nq, k], Ip, D [nq, k], I)``: sorted part lists with integer scores out of a handful of values (L2: 0.0
    among them), ids unique across the parts (some beyond 2^31), pads at the tail, in every other query one part
    entirely pads where there is more than one; and the numpy merge of their union."""
    rng = np.random.default_rng(seed)
    pad = -lc.FLT_MAX if metric == 0 else lc.FLT_MAX
    Dp = np.full((G, nq, k), pad, dtype=np.float32)
    Ip = np.full((G, nq, k), -1, dtype=np.int64)
    D = np.full((nq, k), pad, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for j in range(nq):
        # (every other query: with two parts an all-pad part leaves nothing to merge, the odd queries have both)
        empty = int(rng.integers(G)) if G > 1 and j % 2 == 0 else -1
        lens = [0 if g == empty else int(rng.choice([k, k, max(k - 1, 0), k // 2, 1])) for g in range(G)]
        lens[0 if empty != 0 else 1] = k                                  # (one part is full)
        if G == 1 and j % 5 == 4:
            lens = [0]                                                    # a query with nothing at all
        total = sum(lens)
        ids = rng.choice(1 << 20, size=total, replace=False).astype(np.int64) * 4099 + int(rng.integers(4099))
        sc = rng.integers(0, 6, size=total).astype(np.float64) if metric == 1 else rng.integers(-3, 3, size=total).astype(np.float64)
        if metric == 1 and total:
            sc[0] = 0.0                                                   # an L2 distance of 0.0 in every query
        at = 0
        for g in range(G):
            s_, i_ = sc[at:at + lens[g]], ids[at:at + lens[g]]
            at += lens[g]
            o = np.lexsort((i_, -s_ if metric == 0 else s_))
            Dp[g, j, :lens[g]], Ip[g, j, :lens[g]] = s_[o], i_[o]
        o = np.lexsort((ids, -sc if metric == 0 else sc))[:k]
        D[j, :o.size], I[j, :o.size] = sc[o], ids[o]
    return Dp, Ip, D, I


@pytest.mark.parametrize("k", [1, 64, 128, 129, 2048])
@pytest.mark.parametrize("G", [1, 2, 8])
def test_merge_kernels_on_made_up_parts_equal_the_numpy_merge(G, k):
    import torch

    from claude_semantic_search_amd.sharded import packed_layout

    st = torch.cuda.current_stream().cuda_stream
    for metric in (0, 1):
        for nq in (1, 37):
            Dp, Ip, D, I = _made_up_parts(G, k, nq, metric, seed=G * 10000 + k * 10 + nq + metric)
            if metric == 1:
                assert (Dp == 0.0).any()
            what = f"G={G} k={k} nq={nq} metric={metric}"
            lc.assert_exact(*_merge_dense(torch.from_numpy(Dp).cuda(), torch.from_numpy(Ip).cuda(), nq, k, metric, st), D, I,
                            "dense " + what)
            ib, db, record = packed_layout(nq, k)
            rec = np.zeros((G, record), dtype=np.uint8)
            for g in range(G):
                rec[g, :ib] = Ip[g].reshape(-1).view(np.uint8)
                rec[g, ib:db] = Dp[g].reshape(-1).view(np.uint8)
            lc.assert_exact(*_merge_packed(torch.from_numpy(rec).cuda(), record, nq, k, metric, st), D, I, "packed " + what)


# ---- a size where the paths choose themselves -------------------------------------------------------------------------------
def test_100k_rows_auto_mode_takes_its_own_paths_and_stays_exact():
    """100 000 x 768 rows of family T, inner product, ``auto``: 12 queries take the int8-MFMA sweep and 33 the batch
    cascade by themselves (the scopes tests/test_knn_gpu.py::test_three_to_sixteen_queries_sweep_on_the_int8_mfma asserts);
    1 and 3 queries take the one-launch and the per-stage sweep cascade.  The only case above 20 000 rows: its time is the
    upload and the CPU truth."""
    from claude_semantic_search_amd import _native as nat
    from claude_semantic_search_amd.flat_index import IndexFlatIP

    n, d, k = 100_000, 768, 10
    x, q = lc.case("T", n, d)
    ix = IndexFlatIP(d)
    ix.add(x)
    S = lc.scores64(x, q[:33], 0)
    Dt, It = lc.topk_of_scores(S, k, 0)
    for nq, scope in ((1, None), (3, None), (12, "knn_sweep_mfma_main"), (33, "knn_scan_coarse_main")):
        nat.prof_reset()
        nat.prof_enable(True)
        D, I = ix.search(q[:nq], k)
        nat.prof_enable(False)
        if scope is not None:
            assert nat.prof_read(scope)[1] == 1, f"{nq} queries did not take {scope}"
        lc.assert_exact(D, I, Dt[:nq], It[:nq], f"100k rows, auto, nq={nq}")
    nat.prof_reset()
    ix.close()
