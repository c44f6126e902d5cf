"""Lattice rows: inputs on which every search path must return the same BITS.

Rows and queries of family T have components in {-1, 0, 1}, those of family E components in {-8 .. 8} / 8, and the
searches run with ``normalize=False``.  Every product and every partial sum of an inner product is then an integer (E: a
multiple of 1/64) far below 2^24 for d <= 1024, so an fp32 sum in ANY order is exact; so are the bf16 copies of the
rows, the bf16 MFMA accumulation and the split operands (hi exact, lo = 0).  Squared L2 is exact too, from differences
and in the expanded form ``||q||^2 - 2 x.q + ||x||^2``.  The truth below is therefore not "close to" what a kernel may
return but equal to it: ``D`` under ``np.array_equal`` and ``I`` the order of ``np.lexsort((id, -score))`` -- best score
first, ties to the lower id (include/css_hip.h) -- with no tolerance, no tie window and no excluded slot.  Ties are
everywhere: the scores of T at d = 768 lie within about +-85 over 20 000 rows (tests/test_knn_lattice_host.py counts them).

Plain module like ``knn_checks.py``; nothing here touches the GPU."""
import numpy as np

METRIC_IP, METRIC_L2 = 0, 1
FLT_MAX = np.finfo(np.float32).max
COPIES = 40


def family_T(n, d, seed):
    """``[n, d]`` float32 with components in {-1, 0, 1}."""
    return np.random.default_rng(seed).integers(-1, 2, size=(n, d)).astype(np.float32)


def family_E(n, d, seed):
    """``[n, d]`` float32 with components in {-8 .. 8} / 8 (exact in bf16; NOT exact in int8: 0.125 * 127 is no integer)."""
    return (np.random.default_rng(seed).integers(-8, 9, size=(n, d)) / 8.0).astype(np.float32)


FAMILIES = {"T": family_T, "E": family_E}


def planted(n):
    """Where ``lattice_rows`` plants: ``(zero row, copied row, first row of the block of COPIES copies)``."""
    return n // 3, n // 20, n - n // 4


def lattice_rows(family, n, d, seed):
    """Rows of ``family`` with one all-zero row and, far from its source in id, a block of 40 copies of one row."""
    x = FAMILIES[family](n, d, seed)
    zero, src, blk = planted(n)
    assert src + 1 < zero < blk and blk + COPIES <= n
    x[zero] = 0.0
    x[blk:blk + COPIES] = x[src]
    return x


def lattice_queries(family, nq, d, seed):
    return FAMILIES[family](nq, d, seed)


NQ_MAX = 300


def case(family, n, d):
    """THE rows and the 300 queries of one (family, n, d): the host file measures the ties of exactly what the GPU file
    searches.  Smaller batches are a prefix of the queries."""
    seed = {"T": 1000, "E": 2000}[family] + n % 997 + d
    return lattice_rows(family, n, d, seed), lattice_queries(family, NQ_MAX, d, seed + 1)


def scores64(x, q, metric):
    """``[nq, n]`` float64 scores, exact on lattice inputs: inner products, or squared L2 distances."""
    x64, q64 = np.asarray(x, dtype=np.float64), np.asarray(q, dtype=np.float64).reshape(-1, np.shape(x)[1])
    s = q64 @ x64.T
    if metric == METRIC_L2:
        s = (q64 * q64).sum(1)[:, None] - 2.0 * s + (x64 * x64).sum(1)[None, :]
    return s


def topk_of_scores(S, k, metric, allow=None, exclude=None, id_base=0):
    """The total order of the C ABI applied to a score matrix ``S[nq, n]`` (float64): ``(D float32 [nq, k], I int64)``,
    best first, equal scores by ascending id, pads ``-1`` with ``-FLT_MAX`` (inner product) / ``+FLT_MAX`` (L2) as
    ``search`` pads.  ``allow``: boolean ``[n]``; ``exclude``: per query one LOCAL row that is left out (``-1``: none)."""
    S = np.asarray(S, dtype=np.float64)
    nq, n = S.shape
    key = -S if metric == METRIC_IP else S.copy()       # smaller key = better
    if metric == METRIC_IP:
        key = key + 0.0                                 # (-0.0 -> 0.0: one key per score)
    out = np.zeros((nq, n), dtype=bool)
    if allow is not None:
        out |= ~np.asarray(allow, dtype=bool)[None, :]
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64).reshape(nq)
        rows = np.flatnonzero(ex >= 0)
        out[rows, ex[rows]] = True
    key[out] = np.inf
    ids = np.broadcast_to(np.arange(n, dtype=np.int64), (nq, n))
    kk = min(k, n)
    order = np.lexsort((ids, key), axis=-1)[:, :kk]
    D = np.full((nq, k), -FLT_MAX if metric == METRIC_IP else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    live = ~np.take_along_axis(out, order, axis=1)
    D[:, :kk][live] = np.take_along_axis(S, order, axis=1)[live].astype(np.float32)
    I[:, :kk][live] = order[live] + id_base
    return D, I


def truth_topk(x, q, k, metric, allow=None, exclude=None):
    """Exact top-k of lattice rows: float64 matmul (exact here), order by lexsort; ``(D float32, I int64)``."""
    return topk_of_scores(scores64(x, q, metric), k, metric, allow=allow, exclude=exclude)


def range_of_scores(S, radius, metric, allow=None):
    """``(lims int64 [nq + 1], D float32, I int64)`` of a score matrix under the STRICT predicate of css_hip.h: a row hits
    when ``score > radius`` (inner product) / ``distance < radius`` (L2); a row exactly at the radius does not.  Hits are
    ordered best first, then by ascending id.  The radius is the float32 the library is given."""
    S = np.asarray(S, dtype=np.float64)
    r = np.float64(np.float32(radius))
    hit = S > r if metric == METRIC_IP else S < r
    if allow is not None:
        hit &= np.asarray(allow, dtype=bool)[None, :]
    lims = np.zeros(S.shape[0] + 1, dtype=np.int64)
    Ds, Is = [], []
    for j in range(S.shape[0]):
        ids = np.flatnonzero(hit[j])
        s = S[j, ids]
        order = np.lexsort((ids, -s if metric == METRIC_IP else s))
        Ds.append(s[order].astype(np.float32))
        Is.append(ids[order].astype(np.int64))
        lims[j + 1] = lims[j] + ids.size
    return lims, np.concatenate(Ds) if Ds else np.zeros(0, np.float32), np.concatenate(Is) if Is else np.zeros(0, np.int64)


def truth_range(x, q, radius, metric, allow=None):
    return range_of_scores(scores64(x, q, metric), radius, metric, allow=allow)


def assert_exact(D, I, Dt, It, what=""):
    """Shapes equal, both arrays equal under ``np.array_equal``, every row's non-pad ids unique; a failure names the
    first differing (row, slot) with both (score, id) pairs."""
    D, I, Dt, It = np.asarray(D), np.asarray(I), np.asarray(Dt), np.asarray(It)
    assert D.shape == Dt.shape and I.shape == It.shape, f"{what}: shapes {D.shape} {I.shape}, truth {Dt.shape} {It.shape}"
    if not (np.array_equal(I, It) and np.array_equal(D, Dt)):
        bad = np.argwhere((I != It) | ~(D == Dt))
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {I.size} slots differ, first at {at}: got (score {D[at]!r}, id {int(I[at])}), "
                             f"truth (score {Dt[at]!r}, id {int(It[at])})")
    if I.ndim > 1:                                      # (a flat hit list is cut into queries by its caller)
        for r, row in enumerate(I.reshape(-1, I.shape[-1])):
            ids = row[row >= 0]
            assert np.unique(ids).size == ids.size, f"{what}: row {r} repeats an id"


def assert_exact_range(got, truth, what=""):
    """``(lims, D, I)`` of a range search against ``truth_range``; ids unique inside every query."""
    lims, D, I = got
    lt, Dt, It = truth
    assert np.array_equal(np.asarray(lims), lt), f"{what}: lims differ: {np.asarray(lims).tolist()[:8]} vs {lt.tolist()[:8]}"
    assert_exact(D, I, Dt, It, what)
    for j in range(len(lt) - 1):
        seg = np.asarray(I)[lt[j]:lt[j + 1]]
        assert np.unique(seg).size == seg.size, f"{what}: query {j} repeats an id"


def tie_profile(x, q, ks, metric):
    """Per ``k``: ``{"at_k": share of the queries whose k-th and (k+1)-th true scores are equal, "at_128" / "at_256":
    likewise at ranks 128 and 256 when ``k`` exceeds them, "groups": mean number of groups of two or more equal scores
    inside the list}``."""
    S = scores64(x, q, metric)
    srt = np.sort(-S if metric == METRIC_IP else S, axis=1)
    out = {}
    for k in ks:
        p = {"at_k": float((srt[:, k - 1] == srt[:, k]).mean()) if k < srt.shape[1] else 0.0}
        for b in (128, 256):
            if k > b:
                p[f"at_{b}"] = float((srt[:, b - 1] == srt[:, b]).mean())
        groups = []
        for row in srt[:, :k]:
            _, counts = np.unique(row, return_counts=True)
            groups.append(int((counts >= 2).sum()))
        p["groups"] = float(np.mean(groups))
        out[k] = p
    return out
