"""Float64 restatements of two encoder stages -- the QKV projection and the bf16 attention -- with per-element error
bounds derived from the rounding points of the kernels (test support; numpy only, no GPU).

The bf16 product kernels are otherwise only seen through a pooled 768-vector.  Here a ONE-layer model is run, the
layer's qkv and ctx buffers are read back (``MpnetEncoder.debug_read``), and

* ``attention64`` recomputes ctx from the DEVICE's own qkv bits (teacher forcing: an error of the GEMM cannot hide an
  error of the attention or the other way round), and
* ``qkv64`` recomputes qkv from the token ids with the operands as the device stores them (bf16 copies of the weights,
  bf16 LayerNorm rows or the folded weights of ``k_fold_ln``).

Both return ``(reference, tolerance)`` per element.  The tolerances have no fitted factor: each term is a count of
roundings read from the kernel source times the magnitude it acts on (see the two functions).  ``MUTANTS`` are
deliberately wrong references -- the one-line kernel mistakes these tests exist for; the host test proves each of them
exceeds the bound on the inputs the GPU test uses.

Kernel sources: ``claude_semantic_search_amd/csrc/css_encoder_kernels.h`` (``k_embed_ln``, ``k_embed_pre``,
``k_fold_ln``, ``row_stats_decode``, ``k_gemm`` / ``k_gemm_skinny`` / ``k_gemm8p<EPI_AFF_QKV>`` epilogues, ``attn_pass``,
``k_attention_bf16``) and ``css_encoder.hip`` (``qk_scale``, ``k_build_bias_tab``, ``k_add_row``)."""
from __future__ import annotations

import functools
import math
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from claude_semantic_search_amd import synth

LOG2E = 1.44269504088896341
U_BF16 = 2.0 ** -8     # unit roundoff of a round-to-nearest bf16 conversion (8 significant bits)
U_F32 = 2.0 ** -24     # unit roundoff of one IEEE fp32 operation


# ------------------------------------------------------------------------------------------------ exact roundings
def f32(x) -> np.ndarray:
    """What ONE IEEE fp32 operation returns for the exact result ``x`` (round to nearest even), as float64."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def bf16_ulp(x) -> np.ndarray:
    """Spacing of the bf16 numbers around ``x`` (normal range)."""
    _, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, e - 8)


def bf16_rne(x) -> np.ndarray:
    """Round-to-nearest-even bf16 conversion (``f2bf``: v_cvt_pk_bf16_f32) of ``x``, as float64.  8 significant bits:
    x = m 2^e with m in [0.5, 1) rounds to rint(m 2^8) 2^(e - 8); rint is half-to-even and every step is exact in
    float64.  (Normal range only: the encoder's activations are nowhere near 2^-126.)"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)


def bf16_ambiguous(x, err) -> np.ndarray:
    """Elements of ``x`` (float64) within ``err`` of a bf16 rounding boundary -- the midpoint of two neighbouring bf16
    numbers: a device value that differs from ``x`` by up to ``err`` may round to the other neighbour."""
    x = np.asarray(x, dtype=np.float64)
    ulp = bf16_ulp(x)
    r = np.abs(x) / ulp
    return np.abs(r - np.floor(r) - 0.5) * ulp <= err


# ------------------------------------------------------------------------------------------------ blocked layout
def preblk_elem(t, c, W):
    """Element index of (token t, column c) in a blocked tensor of width W (``preblk_elem``, css_encoder_kernels.h):
    blocks of 16 tokens x 64 columns, inside a block 16-byte pieces in the accumulator order of the producing wave."""
    t = np.asarray(t, dtype=np.int64)
    c = np.asarray(c, dtype=np.int64)
    rowstride = (W >> 6) * 2048                     # bytes from one 16-token block row to the next
    return (((t >> 4) * rowstride + (c >> 6) * 2048) // 2 + ((c >> 5) & 1) * 512 + ((c & 15) >> 2) * 128 + (t & 15) * 8
            + ((c >> 4) & 1) * 4 + (c & 3))


def blocked_numel(T: int, W: int) -> int:
    """Elements to read of a blocked [T, W] tensor: whole 16-token block rows."""
    return (T + 15) // 16 * 16 * W


def deblock(flat, T: int, W: int) -> np.ndarray:
    """Row-major [T, W] view of a blocked tensor read as ``flat`` (at least ``blocked_numel(T, W)`` elements)."""
    flat = np.asarray(flat).reshape(-1)
    return flat[preblk_elem(np.arange(T)[:, None], np.arange(W)[None, :], W)]


# ------------------------------------------------------------------------------------------------ relative position bias
def rel_bucket(rel: int, num_buckets: int = 32, max_distance: int = 128) -> int:
    """Bucket of rel = key - query, from the published definition (T5 / MPNet ``relative_position_bucket``): half the
    buckets per sign, the first ``half / 2`` distances exact, then ``max_exact + floor(log(n / max_exact) /
    log(max_distance / max_exact) (half - max_exact))`` capped at ``half - 1``.  The logarithm is evaluated in integers:
    for the default 32 / 128 it is floor(2 log2(n / 8)) = floor(log2(n^2 / 64)), the bit length of n^2 >> 6 minus one."""
    assert num_buckets == 32 and max_distance == 128, "the integer form below is the 32-bucket / 128-distance case"
    n = -int(rel)
    half = num_buckets // 2
    ret = half if n < 0 else 0
    n = abs(n)
    max_exact = half // 2
    if n < max_exact:
        return ret + n
    return ret + min(max_exact + ((n * n) >> 6).bit_length() - 1, half - 1)


def bias_table(rel_w, heads: int, maxL: int) -> np.ndarray:
    """``bias_tab[h][rel + maxL - 1] = fp32(log2(e)) * W_rel[bucket(rel)][h]`` as ``k_build_bias_tab`` forms it: one fp32
    multiplication, reproduced bit for bit.  rel = key - query."""
    rel_w = np.asarray(rel_w, dtype=np.float64)
    bucket = np.array([rel_bucket(r) for r in range(-(maxL - 1), maxL)])
    return f32(f32(LOG2E) * rel_w[bucket, :heads].T)


def qk_scale(head_dim: int) -> float:
    """The fp32 value ``qk_scale`` (css_encoder.hip) folds into the q columns in bf16 mode: 1 / sqrt(head_dim) times
    log2(e), each step one fp32 operation."""
    s = f32(1.0 / f32(math.sqrt(float(head_dim))))
    return float(f32(s * f32(LOG2E)))


# ------------------------------------------------------------------------------------------------ attention
def attention_delta_ops(head_dim: int, L: int, safe: bool) -> int:
    """Roundings of magnitude <= m_i on one score (``attn_pass``).  Both passes: the fp32 bias table entry, head_dim
    fp32 accumulations of exact bf16 products (an upper count: the MFMA rounds at most once per product), the start
    value and the final sum -- head_dim + 3.  The running-maximum pass (SAFE) adds: the accumulator starts at
    ``bl[..] - mrun`` and every partial sum carries -mrun, |mrun| <= m_i (head_dim + 1 more roundings of magnitude
    m_i), ``s[r] -= d`` (1), and ``mrun += d`` once per 32-key sub-tile at the most, whose rounding is the
    inconsistency between the exact rescale exp2(-d) and the reference later tiles subtract (ceil(L / 32)).
    (css_encoder_kernels.h as of this test: the start value :1588, ``s[r] -= d`` :1625, ``mrun += d`` :1626.)"""
    return head_dim + 3 + ((head_dim + 2 + (L + 31) // 32) if safe else 0)


def attention64(qkv, cu, heads: int, head_dim: int, bias_tab=None, safe: bool = False, probs: Optional[Callable] = None,
                _v: Optional[dict] = None):
    """ctx of one attention layer from the device's own qkv, in float64, with its per-element bound.

    ``qkv`` [T, 3 H] holds the bf16 values the device stored (q already in log2 units: the GEMM epilogue multiplied it
    by ``qk_scale``), ``cu`` the sequence offsets, ``bias_tab`` [heads][2 maxL - 1] the log2-domain table (None: BERT).
    Per sequence, head h and query i, with s_ij = q_i . k_j + b_ij evaluated under a per-row shift:

        ref_id = sum_j 2^s_ij v_jd / sum_j 2^s_ij        A_id = sum_j 2^s_ij |v_jd| / sum_j 2^s_ij
        m_i = max_j (sum_d |q_id k_jd| + |b_ij|)

        tol_id = u |ref_id| + (u + gamma_L + 2^(2 delta_i) - 1) A_id,     u = 2^-8,
        gamma_L = (2 L + 16) 2^-24,   delta_i = attention_delta_ops(head_dim, L, safe) 2^-24 m_i

    u |ref|: the output rounding (``f2bf(oacc * inv)``).  u A: ``(__bf16)s[..]`` -- p is rounded to bf16 before the P.V
    MFMA while the denominator sums the fp32 p.  gamma_L: fp32 accumulation of P.V (L) and of the row sum (L),
    ``v_exp_f32`` (2 ulp = 4), the reciprocal and the product with it (2), the rescales of the guarded pass and the
    cross-half add (<= 10).  delta_i: the absolute error of a log2-domain score; it multiplies a term of the numerator
    and of the denominator by up to 2^(+-delta) each.

    Returns ``(ref [T, H], tol [T, H], log2sum [T, heads])``; ``log2sum`` is log2 of the un-shifted row sum (what the
    fast pass holds in fp32).  ``probs(b, h, P)`` is called with each [L, L] probability matrix when given."""
    qkv = np.asarray(qkv, dtype=np.float64)
    cu = np.asarray(cu, dtype=np.int64)
    H = heads * head_dim
    T = int(cu[-1])
    v_ = _v or {}
    ref = np.zeros((T, H))
    tol = np.zeros((T, H))
    log2sum = np.zeros((T, heads))
    maxL = (bias_tab.shape[1] + 1) // 2 if bias_tab is not None else 0
    for b in range(len(cu) - 1):
        t0, t1 = int(cu[b]), int(cu[b + 1])
        L = t1 - t0
        keys = np.arange(L)
        if v_.get("drop_last") and L >= 2:
            keys = keys[:-1]
        if v_.get("drop_mod64") is not None and L >= 2:
            keys = keys[keys % 64 != v_["drop_mod64"]]
        ktok = t0 + keys
        krel = keys.astype(np.int64)
        if v_.get("next_seq_key") and t1 < T:       # the token behind the sequence read as key L
            ktok = np.append(ktok, t1)
            krel = np.append(krel, L)
        for h in range(heads):
            q = qkv[t0:t1, h * head_dim:(h + 1) * head_dim]
            if v_.get("no_log2e"):
                q = q / LOG2E
            k = qkv[ktok, H + h * head_dim:H + (h + 1) * head_dim]
            hv = h ^ 1 if v_.get("swap_v_heads") else h
            v = qkv[ktok, 2 * H + hv * head_dim:2 * H + (hv + 1) * head_dim]
            s = q @ k.T
            mag = np.abs(q) @ np.abs(k).T
            if bias_tab is not None:
                rel = krel[None, :] - np.arange(L)[:, None]
                rel = v_.get("rel_sign", 1) * rel + v_.get("rel_shift", 0)
                bb = bias_tab[h][np.clip(rel + maxL - 1, 0, 2 * maxL - 2)]
                s = s + bb
                mag = mag + np.abs(bb)
            shift = s.max(axis=1, keepdims=True)
            w = np.exp2(s - shift)
            den = w.sum(axis=1, keepdims=True)
            r = (w @ v) / den
            A = (w @ np.abs(v)) / den
            m = mag.max(axis=1, keepdims=True)
            delta = attention_delta_ops(head_dim, L, safe) * U_F32 * m
            gamma = (2 * L + 16) * U_F32
            ref[t0:t1, h * head_dim:(h + 1) * head_dim] = r
            tol[t0:t1, h * head_dim:(h + 1) * head_dim] = U_BF16 * np.abs(r) + (U_BF16 + gamma + np.exp2(2 * delta) - 1) * A
            log2sum[t0:t1, h] = (shift + np.log2(den))[:, 0]
            if probs is not None:
                probs(b, h, w / den)
        if v_.get("swap_qblocks") and L > 128:       # query blocks 0 and 1 exchanged where both rows exist
            n = min(128, L - 128)
            blk = ref[t0:t0 + n].copy()
            ref[t0:t0 + n] = ref[t0 + 128:t0 + 128 + n]
            ref[t0 + 128:t0 + 128 + n] = blk
    return ref, tol, log2sum


EDGE_POSITIONS = (0, 31, 32, 63, 64, 127, 128)


def edge_positions(L: int) -> List[int]:
    """Key / query positions at the 32- and 64-key tile edges, the 128-query block edge and the sequence end."""
    return sorted({p for p in EDGE_POSITIONS + (L - 1,) if 0 <= p < L})


def edge_coverage(qkv, cu, heads: int, head_dim: int, bias_tab=None, pmin: float = 0.25) -> List[str]:
    """The edge-coverage condition on a qkv tensor: for every sequence and every edge KEY position some (head, query)
    gives it probability >= pmin, and every edge QUERY position has a head whose largest probability is >= pmin (a
    wrong or missing key then moves an output by a multiple of the bound).  Returns the violations (empty: holds)."""
    cu = np.asarray(cu, dtype=np.int64)
    best_key: Dict[int, np.ndarray] = {}
    best_qry: Dict[int, np.ndarray] = {}

    def see(b, h, P):
        best_key[b] = np.maximum(best_key.get(b, 0.0), P.max(axis=0))
        best_qry[b] = np.maximum(best_qry.get(b, 0.0), P.max(axis=1))

    attention64(qkv, cu, heads, head_dim, bias_tab, probs=see)
    bad = []
    for b in range(len(cu) - 1):
        L = int(cu[b + 1] - cu[b])
        for p in edge_positions(L):
            if best_key[b][p] < pmin:
                bad.append(f"L={L}: key {p} never reaches p >= {pmin} (best {best_key[b][p]:.3f})")
            if best_qry[b][p] < pmin:
                bad.append(f"L={L}: query {p} has no probability >= {pmin} (best {best_qry[b][p]:.3f})")
    return bad


# ------------------------------------------------------------------------------------------------ QKV projection
# Roundings of the fp32 LayerNorm of k_embed_ln, per quantity (each `+` / `*` below is one fp32 operation):
LN_SUM_OPS = 2 + 3 + 6 + 2      # (x + y) + (z + w): 2; s += over <= 3 float4 per lane: 3; wave_allsum: 6; * (1.0f / H): 2
LN_VAR_OPS = 1 + LN_SUM_OPS + 1  # dx * dx: 1; the same sum; + eps: 1
RSQRT_OPS = 4                   # rsqrtf: within 2 ulp
# k_embed_pre: s1 += x + y over 6 pieces x 4 pairs per thread (25), 16 partial sums in order (16); row_stats_decode:
# int -> float and the fma (2), * (1 / scale) * inv_h (2)
STAT_SUM_OPS = 25 + 16
STAT_DECODE_OPS = 2 + 2


def _fold_ops(K: int) -> int:
    """Roundings of c_j and d_j in k_fold_ln: K / 64 fma per lane, wave_allsum (6), / K or + bias (1)."""
    return K // 64 + 6 + 1


def fused_qkv(w: Dict[str, np.ndarray], arch: str):
    """Fused [3 H, H] weight and [3 H] bias (fp32 values as float64) of layer 0 from a state dict."""
    if arch == "bert":
        names = [f"encoder.layer.0.attention.self.{n}" for n in ("query", "key", "value")]
    else:
        names = [f"encoder.layer.0.attention.attn.{n}" for n in "qkv"]
    W = np.concatenate([np.asarray(w[n + ".weight"], dtype=np.float64) for n in names])
    b = np.concatenate([np.asarray(w[n + ".bias"], dtype=np.float64) for n in names])
    return W, b


def embedding_sum(w: Dict[str, np.ndarray], arch: str, batch: Sequence[Sequence[int]]) -> np.ndarray:
    """fp32(wemb[id] + pemb[pos]) per token, bit for bit (k_embed_ln / k_embed_pre).  MPNet: pos = 2 + offset; BERT: pos
    = offset and the position table first takes token-type row 0 in fp32 (k_add_row)."""
    wemb = np.asarray(w["embeddings.word_embeddings.weight"], dtype=np.float64)
    pemb = np.asarray(w["embeddings.position_embeddings.weight"], dtype=np.float64)
    if arch == "bert":
        pemb = f32(pemb + np.asarray(w["embeddings.token_type_embeddings.weight"], dtype=np.float64)[0])
    ids = np.concatenate([np.asarray(s, dtype=np.int64) for s in batch])
    pos = np.concatenate([np.arange(len(s)) for s in batch]) + (0 if arch == "bert" else 2)
    return f32(wemb[ids] + pemb[pos])


def layernorm64(x, gamma, beta, eps: float):
    """LayerNorm of the rows of ``x`` in float64 and the bound on what k_embed_ln's fp32 arithmetic deviates from it:

        o = (x - mean) rstd g + b
        |mean error| <= LN_SUM_OPS 2^-24 mean|x|                                        (me)
        dx = x - mean: 2^-24 |dx| + me
        rstd: half the relative error of the variance, (2 + LN_VAR_OPS) 2^-24 + 2 me rstd, plus rsqrtf
        o: two products and the add."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=1, keepdims=True)
    dx = x - mean
    var = (dx * dx).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    o = dx * rstd * gamma + beta
    me = LN_SUM_OPS * U_F32 * np.abs(x).mean(axis=1, keepdims=True)
    rel_rstd = 0.5 * (2 + LN_VAR_OPS) * U_F32 + me * rstd + RSQRT_OPS * U_F32
    err = np.abs(gamma) * rstd * (np.abs(dx) * (U_F32 + rel_rstd + 2 * U_F32) + me) + U_F32 * np.abs(o)
    return o, err


def qkv64(w: Dict[str, np.ndarray], arch: str, heads: int, ln_eps: float, batch: Sequence[Sequence[int]], folded: bool,
          exact: bool = False):
    """qkv of layer 0 from the token ids, float64 arithmetic on the operands as the device stores them.

    Row-major path (``folded=False``: k_embed_ln, then k_gemm / k_gemm_skinny with EPI_QKV):
        A = bf16(LN(x)), x = fp32(wemb + pemb);  Wd = bf16(W);  y = (A Wd^T + b) sc_j
    LayerNorm-folded path (``folded=True``: k_embed_pre, k_fold_ln, k_gemm8p<EPI_AFF_QKV>):
        A = bf16(x);  Wd[j,k] = bf16(W[j,k] g[k] - c_j), c_j = mean_k W[j,k] g[k];  d_j = sum_k beta[k] W[j,k] + b_j
        rs_t = 1 / sqrt(sum A^2 / H - (sum A / H)^2 + eps)           (row statistics of the STORED values)
        y = (rs_t (A Wd^T) + d_j) sc_j                               (fma(acc, rs sc, d sc): no mean term, W' is centred)
    sc_j = qk_scale on the q columns, 1 elsewhere.

    Bound (K = hidden, e the fp32 part, every term times sc_j):
        e = (K + 2) 2^-24 (r_t sum_k |a_tk w_jk| + |bias terms|)     K accumulations, the bias add, the scale
          + r_t sum_{k ambiguous} ulp_bf16(.) |other operand|         operands known only up to an fp32 error
          + rho_t r_t |A Wd^T|                                       folded only: the fp32 error of rs (below)
        tol = u (|y| + e) + e                                        the bf16 rounding of the stored value
    with r_t = rs_t (folded) or 1.  Row-major: the ambiguous operands are the LayerNorm outputs within ``layernorm64``'s
    error of a bf16 boundary; |bias terms| = |b_j|.  Folded: the ambiguous operands are the folded weights, whose fp32
    value fma(W, g, -c) carries the error of c (_fold_ops(K) 2^-24 mean|W g|) and its own rounding; |bias terms| =
    sum_k |beta_k W_jk| + |b_j| (d_j: _fold_ops(K) <= K roundings).
    rho_t (k_embed_pre, row_stats_decode): sums of STAT_SUM_OPS fp32 additions, the 2^-24 / 2^-20 fixed-point grids,
    STAT_DECODE_OPS, var = fma(s2, inv_h, -mu^2), + eps, rsqrtf:
        |mu error| <= (STAT_SUM_OPS + STAT_DECODE_OPS) 2^-24 mean|a| + 2^-25 / H
        |var error| <= (STAT_SUM_OPS + STAT_DECODE_OPS + 1) 2^-24 mean(a^2) + 2^-21 / H + 2 |mu| |mu error| + 2^-24 mu^2
                       + 2^-24 |var|
        rho_t = |var error| / (2 (var + eps)) + (1 / 2 + RSQRT_OPS) 2^-24          (+ eps: half a rounding; rsqrtf)
    (css_encoder_kernels.h as of this test: the sums :199-220, row_stats_decode :862-870, the epilogue's
    ``fma(v, rs sc, d sc)`` :1245-1246, k_fold_ln :226-244.)

    ``exact=True`` leaves out the bf16 roundings of the operands: both paths then ARE the model's q / k / v (the host
    test pins them against the oracles that way).

    Returns a dict: ``y``, ``tol`` [T, 3 H]; ``n_ambiguous``; and the operands the mutants need (``A``, ``W``, ``r``,
    ``bias``, ``sc``)."""
    rnd = (lambda a: np.asarray(a, dtype=np.float64)) if exact else bf16_rne
    W, bias = fused_qkv(w, arch)
    K = W.shape[1]
    head_dim = K // heads
    gam = np.asarray(w["embeddings.LayerNorm.weight"], dtype=np.float64)
    bet = np.asarray(w["embeddings.LayerNorm.bias"], dtype=np.float64)
    x = embedding_sum(w, arch, batch)
    T = x.shape[0]
    sc = np.ones(3 * K)
    sc[:K] = qk_scale(head_dim)
    if not folded:
        o, err = layernorm64(x, gam, bet, ln_eps)
        A = rnd(o)
        amb = bf16_ambiguous(o, err)
        Wd = rnd(W)                                   # k_f32_to_bf16 of the fp32 master: exact restatement
        r = np.ones((T, 1))
        dvec = bias
        bias_mag = np.abs(bias)
        amb_term = (amb * bf16_ulp(o)) @ np.abs(Wd).T
        rho = np.zeros((T, 1))
        n_amb = int(amb.sum())
    else:
        A = rnd(x)
        Wg = W * gam
        c = Wg.mean(axis=1, keepdims=True)
        w64 = Wg - c
        err_w = _fold_ops(K) * U_F32 * np.abs(Wg).mean(axis=1, keepdims=True) + U_F32 * np.abs(w64)
        Wd = rnd(w64)
        amb = bf16_ambiguous(w64, err_w)
        dvec = W @ bet + bias
        bias_mag = np.abs(W) @ np.abs(bet) + np.abs(bias)
        mu = A.mean(axis=1, keepdims=True)
        m2 = (A * A).mean(axis=1, keepdims=True)
        var = np.maximum(m2 - mu * mu, 0.0)
        r = 1.0 / np.sqrt(var + ln_eps)
        n_s = STAT_SUM_OPS + STAT_DECODE_OPS
        mu_err = n_s * U_F32 * np.abs(A).mean(axis=1, keepdims=True) + 2.0 ** -25 / K
        var_err = (n_s + 1) * U_F32 * m2 + 2.0 ** -21 / K + 2 * np.abs(mu) * mu_err + U_F32 * mu * mu + U_F32 * var
        rho = 0.5 * var_err / (var + ln_eps) + 0.5 * U_F32 + RSQRT_OPS * U_F32
        amb_term = np.abs(A) @ (amb * bf16_ulp(w64)).T
        n_amb = int(amb.sum())
    S = A @ Wd.T
    y = (r * S + dvec) * sc
    e = sc * ((K + 2) * U_F32 * (r * (np.abs(A) @ np.abs(Wd).T) + bias_mag) + r * amb_term + rho * r * np.abs(S))
    tol = U_BF16 * (np.abs(y) + e) + e
    return dict(y=y, tol=tol, n_ambiguous=n_amb, A=A, W=Wd, r=r, bias=dvec, sc=sc)


# ------------------------------------------------------------------------------------------------ mutants
def _att(**v):
    def run(qkv, cu, heads, head_dim, bias_tab=None):
        return attention64(qkv, cu, heads, head_dim, bias_tab, _v=v)[0]
    return run


def _swap_rows(y, step):
    y = y.copy()
    for b in range(step, y.shape[0], step):
        y[[b - 1, b]] = y[[b, b - 1]]
    return y


def _drop_kstep(p):
    ks = slice(p["A"].shape[1] - 64, p["A"].shape[1] - 32)
    return p["y"] - p["r"] * (p["A"][:, ks] @ p["W"][:, ks].T) * p["sc"]


def _next_bias(p):
    b = np.roll(p["bias"], -1)
    return p["y"] + (b - p["bias"]) * p["sc"]


def _scale_first_k(p):
    y = p["y"].copy()
    H = y.shape[1] // 3
    y[:, H] *= p["sc"][0]
    return y


#: Deliberately wrong references.  "attention": f(qkv, cu, heads, head_dim, bias_tab) -> ctx; "needs": the sequences
#: (length L, is it the batch's last, has the model a bias) the mistake can change.  "qkv": f(qkv64 result) -> y;
#: "needs": the smallest token count T at which it changes anything.
MUTANTS = {
    "attention": {
        "bias mirrored (rel -> -rel)": dict(f=_att(rel_sign=-1), needs=lambda L, last, bias: bias and L >= 2),
        "bias shifted by one position": dict(f=_att(rel_shift=1), needs=lambda L, last, bias: bias and L >= 2),
        "last key of the sequence dropped": dict(f=_att(drop_last=True), needs=lambda L, last, bias: L >= 2),
        "first key of each 64-key tile dropped": dict(f=_att(drop_mod64=0), needs=lambda L, last, bias: L >= 2),
        "first key of each second 32-key half dropped": dict(f=_att(drop_mod64=32), needs=lambda L, last, bias: L >= 33),
        "next sequence's first token added as a key": dict(f=_att(next_seq_key=True), needs=lambda L, last, bias: not last),
        "q scale without log2(e)": dict(f=_att(no_log2e=True), needs=lambda L, last, bias: L >= 2),
        "query blocks of 128 swapped": dict(f=_att(swap_qblocks=True), needs=lambda L, last, bias: L > 128),
        "heads h and h + 1 swapped for v": dict(f=_att(swap_v_heads=True), needs=lambda L, last, bias: True),
    },
    "qkv": {
        "one 32-column K step dropped": dict(f=_drop_kstep, needs=1),
        "rows exchanged at each 16-row boundary": dict(f=lambda p: _swap_rows(p["y"], 16), needs=17),
        "rows exchanged at each 64-row boundary": dict(f=lambda p: _swap_rows(p["y"], 64), needs=65),
        "rows exchanged at each 128-row boundary": dict(f=lambda p: _swap_rows(p["y"], 128), needs=129),
        "bias of column j + 1 used for column j": dict(f=_next_bias, needs=1),
        "q scale applied to the first k column": dict(f=_scale_first_k, needs=1),
    },
}


# ------------------------------------------------------------------------------------------------ the test inputs
#: One-layer models, vocabulary 1000.  qk_gain multiplies the q and k weights and biases ("fast": log2-domain scores
#: of standard deviation ~8, |score| <= 60, every row sum inside 2^+-60; "fallback": logits in the hundreds, row sums
#: outside the fast pass's 2^+-100 window); rel_gain multiplies the relative-bias table (standard deviation ~1.5).
MODELS = {
    "mpnet768": dict(arch="mpnet", hidden=768, heads=12, ffn=3072, max_pos=514, max_seq_len=384, ln_eps=1e-5, seed=41,
                     qk_gain=dict(fast=4.2, fallback=15.0), rel_gain=15.0),
    "bert768": dict(arch="bert", hidden=768, heads=12, ffn=3072, max_pos=512, max_seq_len=512, ln_eps=1e-12, seed=42,
                    qk_gain=dict(fast=4.2, fallback=15.0), rel_gain=None),
    "bert384": dict(arch="bert", hidden=384, heads=12, ffn=1536, max_pos=512, max_seq_len=512, ln_eps=1e-12, seed=43,
                    qk_gain=dict(fast=6.0, fallback=21.0), rel_gain=None),
}
VOCAB = 1000
_BASE = [383, 1, 129, 31, 64, 2, 384, 33, 63, 127, 65, 128, 32]          # 1442 tokens; sequences start off the 16-grid
#: batches of sequence lengths (every length is used once per model: a sequence is named by its length)
BATCHES = {
    "mpnet768": dict(big=[_BASE], small=[_BASE[:6], _BASE[6:]]),
    "bert768": dict(big=[[511, 1, 2, 31, 512], [383, 129, 64, 384, 33, 63, 127, 65, 128, 32]],
                    small=[[512, 1, 129, 31, 64, 2], [511, 33, 63, 127, 65, 128, 32], [383, 384]]),
}
BATCHES["bert384"] = BATCHES["bert768"]
#: k_gemm_skinny<.., 1> (<= 32 tokens) and <.., 2> (33 .. 64 tokens)
SKINNY = dict(skinny1=[[2, 1], [31, 1]], skinny2=[[33, 2], [63, 1]])


def model_cfg(name: str) -> dict:
    """``cfg_overrides`` of ``MpnetEncoder(synthetic_seed=...)``."""
    m = MODELS[name]
    bert = m["arch"] == "bert"
    return dict(num_layers=1, hidden=m["hidden"], heads=m["heads"], ffn=m["ffn"], vocab=VOCAB, max_pos=m["max_pos"],
                rel_buckets=0 if bert else 32, pad_id=0 if bert else 1, max_seq_len=m["max_seq_len"], ln_eps=m["ln_eps"],
                arch=m["arch"], pooling="mean", normalize=True)


def _tensor(seed, tid, shape, mean, std):
    n = int(np.prod(shape))
    v = synth.normal(synth.tensor_seed(seed, tid), np.arange(n, dtype=np.uint64))
    return (np.float32(mean) + np.float32(std) * v).astype(np.float32).reshape(shape)


@functools.lru_cache(maxsize=None)
def model_weights(name: str, kind: str = "fast") -> Dict[str, np.ndarray]:
    """State dict (fp32 numpy, HF names) of a test model: the synthetic distributions of the encoder (weights N(0,
    0.02^2), biases N(0, 0.05^2), LayerNorm gamma N(1, 0.1^2) / beta N(0, 0.05^2), relative bias N(0, 0.1^2)) with the
    q / k and relative-bias gains of ``MODELS``."""
    m = MODELS[name]
    H, Fd, seed, bert = m["hidden"], m["ffn"], m["seed"], m["arch"] == "bert"
    w: Dict[str, np.ndarray] = {}
    w["embeddings.word_embeddings.weight"] = _tensor(seed, 0, (VOCAB, H), 0.0, 0.02)
    w["embeddings.position_embeddings.weight"] = _tensor(seed, 1, (m["max_pos"], H), 0.0, 0.02)
    w["embeddings.LayerNorm.weight"] = _tensor(seed, 2, (H,), 1.0, 0.1)
    w["embeddings.LayerNorm.bias"] = _tensor(seed, 3, (H,), 0.0, 0.05)
    if bert:
        w["embeddings.token_type_embeddings.weight"] = _tensor(seed, 5, (2, H), 0.0, 0.02)
        p = "encoder.layer.0.attention."
        names = dict(q=p + "self.query", k=p + "self.key", v=p + "self.value", o=p + "output.dense", ln=p + "output.LayerNorm")
    else:
        w["encoder.relative_attention_bias.weight"] = _tensor(seed, 4, (32, m["heads"]), 0.0, 0.1) * np.float32(m["rel_gain"])
        p = "encoder.layer.0.attention."
        names = dict(q=p + "attn.q", k=p + "attn.k", v=p + "attn.v", o=p + "attn.o", ln=p + "LayerNorm")
    g = np.float32(m["qk_gain"][kind])
    for j, nm in enumerate("qkv"):
        gain = g if nm in "qk" else np.float32(1.0)
        w[names[nm] + ".weight"] = _tensor(seed, 16 + 2 * j, (H, H), 0.0, 0.02) * gain
        w[names[nm] + ".bias"] = _tensor(seed, 17 + 2 * j, (H,), 0.0, 0.05) * gain
    w[names["o"] + ".weight"] = _tensor(seed, 22, (H, H), 0.0, 0.02)
    w[names["o"] + ".bias"] = _tensor(seed, 23, (H,), 0.0, 0.05)
    w[names["ln"] + ".weight"] = _tensor(seed, 24, (H,), 1.0, 0.1)
    w[names["ln"] + ".bias"] = _tensor(seed, 25, (H,), 0.0, 0.05)
    q = "encoder.layer.0."
    w[q + "intermediate.dense.weight"] = _tensor(seed, 26, (Fd, H), 0.0, 0.02)
    w[q + "intermediate.dense.bias"] = _tensor(seed, 27, (Fd,), 0.0, 0.05)
    w[q + "output.dense.weight"] = _tensor(seed, 28, (H, Fd), 0.0, 0.02)
    w[q + "output.dense.bias"] = _tensor(seed, 29, (H,), 0.0, 0.05)
    w[q + "output.LayerNorm.weight"] = _tensor(seed, 30, (H,), 1.0, 0.1)
    w[q + "output.LayerNorm.bias"] = _tensor(seed, 31, (H,), 0.0, 0.05)
    return w


#: Draw of a sequence's token ids, where the first draw (0) leaves an edge key or query without a probability >= 0.35
#: on the reference chain (found on the CPU; tests/test_encoder_stages_host.py holds the condition itself)
SEQ_DRAW: Dict[str, Dict[int, int]] = {"mpnet768": {}, "bert768": {384: 1}, "bert384": {128: 1, 383: 2, 384: 1, 511: 3}}


def sequence_ids(name: str, L: int, draw: Optional[int] = None) -> List[int]:
    """Token ids of the model's sequence of length L: uniform in [3, VOCAB) (never a pad id)."""
    draw = SEQ_DRAW[name].get(L, 0) if draw is None else draw
    idx = np.arange(L, dtype=np.uint64) + np.uint64(L) * np.uint64(1 << 20) + np.uint64(draw) * np.uint64(1 << 40)
    return synth.uint(MODELS[name]["seed"], idx, 3, VOCAB).tolist()


def batch_ids(name: str, lengths: Sequence[int]) -> List[List[int]]:
    return [sequence_ids(name, L) for L in lengths]


def offsets(lengths: Sequence[int]) -> np.ndarray:
    cu = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=cu[1:])
    return cu


def model_bias_table(name: str, kind: str = "fast"):
    m = MODELS[name]
    if m["arch"] == "bert":
        return None
    return bias_table(model_weights(name, kind)["encoder.relative_attention_bias.weight"], m["heads"], m["max_seq_len"])


def path_is_folded(name: str, lengths: Sequence[int]) -> bool:
    """The forward of this batch takes the LayerNorm-folded path (hidden 768, >= 1024 tokens: blocked qkv / ctx)."""
    return MODELS[name]["hidden"] == 768 and sum(lengths) >= 1024


@functools.lru_cache(maxsize=None)
def reference_qkv(name: str, lengths: tuple, kind: str = "fast") -> dict:
    """``qkv64`` of a batch of the model on the path its forward takes (computed once, shared by the tests)."""
    m = MODELS[name]
    return qkv64(model_weights(name, kind), m["arch"], m["heads"], m["ln_eps"], batch_ids(name, lengths),
                 path_is_folded(name, lengths))
