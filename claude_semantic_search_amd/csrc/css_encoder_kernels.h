// css_encoder_kernels.h -- device kernels of the MPNet encoder (gfx950).
//
// Math follows SURVEY.md Appendix A (validated there against transformers'
// modeling_mpnet.py): embeddings + LN, 12 post-LN layers with a shared T5-style
// relative position bias, masked mean pooling, L2 normalise.
//
// Two compute modes share every kernel template:
//   bf16 (product): GEMM / attention operands in bf16 on v_mfma_f32_32x32x16_bf16,
//        fp32 accumulation; LayerNorm, softmax, residual stream, pooling in fp32.
//   fp32 (verification): same tiling on v_mfma_f32_32x32x2_f32 (exact fp32).
//
// Activations are PACKED var-len: T = sum of sequence lengths rows, no padding.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "css_knn_kernels.h"

namespace css {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef short v8s __attribute__((ext_vector_type(8)));
typedef unsigned short bf16_t;  // storage type of bf16 tensors

__device__ __forceinline__ bf16_t f2bf(float f) {
    __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: round-to-nearest-even, NaN preserving
    return __builtin_bit_cast(bf16_t, b);
}
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }

// 128-byte LDS rows (64 bf16 or 32 f32) with the 16-B chunk index XOR-swizzled by
// (row>>1)&7: every ds_read_b128 lane group then covers 16 distinct slots.
__device__ __forceinline__ int swz_byte(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// ---------------------------------------------------------------- embeddings + LN
// One wave per token.  H = hidden (a multiple of 128): lane handles the float4 columns lane + 64 i; with
// H % 256 != 0 (hidden 384: 96 float4 per row) the lanes of the last round beyond H / 4 hold zeros.
// pos_off: position id of a sequence's first token (MPNet: padding_idx + 1 = 2; BERT: 0, its token-type row 0 is
// folded into the position table at weight-load time).
template <int H>
__device__ __forceinline__ bool ln_col_ok(int idx) {   // float4 column idx of a row exists
    return H % 256 == 0 || idx < H / 4;
}
// Token type of position `rel` of a sequence of `len` tokens in a cross-encoder pair batch (css_encoder_forward_pairs):
// 0 before seg_start, 1 from there on.  seg_start is clamped into [1, len]: the _dev entry point cannot check it.
__device__ __forceinline__ bool seg_type1(const int32_t* __restrict__ seg, int b, int rel, int len) {
    return seg != nullptr && rel >= min(max(seg[b], 1), len);
}
// seg (per sequence, may be NULL) / tdelta [H] = token_type_embeddings[1] - [0]: a type-1 token's row is
// (word + pemb[pos]) + tdelta before the statistics.  seg == NULL: the additions below are those of a plain forward.
template <int H>
__global__ __launch_bounds__(256) void k_embed_ln(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                  int B, const float* __restrict__ wemb,
                                                  const float* __restrict__ pemb, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float eps, int vocab, int max_pos,
                                                  int pos_off, float* __restrict__ out32, bf16_t* __restrict__ out16, int T,
                                                  const int32_t* __restrict__ seg, const float* __restrict__ tdelta) {
    static_assert(H % 128 == 0, "float4 columns of a row cover whole 32-lane halves");
    constexpr int NV = (H / 4 + 63) / 64;  // float4 per lane
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    // sequence of token t: binary search in cu_seqlens
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= t) lo = mid; else hi = mid;
    }
    int id = ids[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int pos = (t - cu[lo]) + pos_off;  // packed (no pads): MPNet cumsum(mask)*mask + padding_idx(1); BERT arange
    pos = pos < max_pos ? pos : max_pos - 1;
    const float4* w4 = reinterpret_cast<const float4*>(wemb + (size_t)id * H);
    const float4* p4 = reinterpret_cast<const float4*>(pemb + (size_t)pos * H);
    const bool ty1 = seg_type1(seg, lo, t - cu[lo], cu[lo + 1] - cu[lo]);   // (wave-uniform: one token per wave)
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float4 a = w4[lane + 64 * i], b = p4[lane + 64 * i];
        v[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        if (ty1) {
            const float4 d = reinterpret_cast<const float4*>(tdelta)[lane + 64 * i];
            v[i] = make_float4(v[i].x + d.x, v[i].y + d.y, v[i].z + d.z, v[i].w + d.w);
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_allsum(s) * (1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = rsqrtf(wave_allsum(q) * (1.0f / H) + eps);
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float4 g = g4[lane + 64 * i], b = b4[lane + 64 * i];
        float4 o;
        o.x = (v[i].x - mean) * rstd * g.x + b.x;
        o.y = (v[i].y - mean) * rstd * g.y + b.y;
        o.z = (v[i].z - mean) * rstd * g.z + b.z;
        o.w = (v[i].w - mean) * rstd * g.w + b.w;
        reinterpret_cast<float4*>(out32 + (size_t)t * H)[lane + 64 * i] = o;
        if (out16) {
            ushort4 h;
            h.x = f2bf(o.x); h.y = f2bf(o.y); h.z = f2bf(o.z); h.w = f2bf(o.w);
            reinterpret_cast<ushort4*>(out16 + (size_t)t * H)[lane + 64 * i] = h;
        }
    }
}

// ---- the BLOCKED layout of the LayerNorm-folded path's `pre` tensors ([T][H] bf16, H % 64 == 0) ---------------------
// A pre tensor is written by k_gemm8p<EPI_RES> and read back by the next EPI_RES GEMM (residual), by the EPI_AFF_* GEMMs
// (A operand through LDS-DMA) and by the pooling.  It is stored in blocks of 16 tokens x 64 columns = 2 KiB, block
// (t >> 4, c >> 6) at byte (t >> 4) * preblk_rowstride(H) + (c >> 6) * 2048, and inside a block in the ACCUMULATOR order of
// the producing wave: 16-byte piece (j, lg, lq) at j * 1024 + lg * 256 + lq * 16 holds token row lq, columns
// 16 (2 j) + 4 lg + {0..3} and 16 (2 j + 1) + 4 lg + {0..3} -- exactly the two v4f accumulators acc[m][2 j], acc[m][2 j + 1]
// of lane lq + 16 lg.  So the producer stores, and the next EPI_RES GEMM re-reads, whole registers with 1-KiB-contiguous
// wave instructions and NO LDS transpose (round 3's row-major pre went through the wave's LDS scratch twice per 16-row
// block: O projection 2.00 ms, 28 % of the bf16 peak).  A consumer GEMM's LDS-DMA fetches 16-byte pieces by per-lane
// addresses anyway; its K-step u = block column u, LDS chunk cl = piece (j = cl >> 2, lg = cl & 3), i.e. the K order
// inside a 64-column block is permuted -- and the consumer's weights carry the same permutation (k_fold_ln, `perm`).
// Bytes from one 16-row block row to the next: the H / 64 blocks, no padding.
__host__ __device__ __forceinline__ size_t preblk_rowstride(int H) { return (size_t)(H >> 6) * 2048; }
// G8_BBLK: the WEIGHTS of the GEMMs with blocked A operands are stored in the blocked layout too ([N][K] through
// preblk_elem: contiguous 1-KiB DMA pieces, fragment reads without a swizzle; 0: row-major with the K order permuted)
#ifndef G8_BBLK
#define G8_BBLK 1
#endif
__device__ __forceinline__ size_t preblk_elem(int t, int c, int H) {   // element index of (token t, column c)
    return ((size_t)(t >> 4) * preblk_rowstride(H) + (size_t)(c >> 6) * 2048) / 2 + ((c >> 5) & 1) * 512 + ((c & 15) >> 2) * 128 +
           (t & 15) * 8 + ((c >> 4) & 1) * 4 + (c & 3);
}
__host__ __device__ __forceinline__ int preblk_kpos(int k) {   // position of original column k in the permuted K order
    const int cc = k & 63;
    return (k & ~63) + ((((cc >> 5) & 1) * 4 + ((cc & 15) >> 2)) << 3) + ((cc >> 4) & 1) * 4 + (cc & 3);
}

// LayerNorm-folded path (k_gemm8p EPI_AFF_* / EPI_RES): the embedding sum is stored un-normalised as bf16 (blocked
// layout above) together with the row sums of the STORED values in the fixed-point format of row_stats_decode.
template <int H>
__global__ __launch_bounds__(256) void k_embed_pre(const int32_t* __restrict__ ids, const int32_t* __restrict__ cu,
                                                   int B, const float* __restrict__ wemb,
                                                   const float* __restrict__ pemb, int vocab, int max_pos, int pos_off,
                                                   bf16_t* __restrict__ pre, long long* __restrict__ stats, int T,
                                                   float scale1, float scale2, const int32_t* __restrict__ seg,
                                                   const float* __restrict__ tdelta) {
    // One block = one 16-token block row of the blocked layout: thread (lq = tid & 15, g = tid >> 4) writes the 16-byte
    // pieces g, g + 16, ... of token lq, so 16 consecutive lanes store 256 contiguous bytes (one piece row of a block).
    static_assert(H % 64 == 0, "blocked layout");
    constexpr int NP = H / 8;   // 16-byte pieces per token row
    __shared__ float red[2][16][17];
    const int lq = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int t = blockIdx.x * 16 + lq;
    float s1 = 0.f, s2 = 0.f;
    if (t < T) {
        int lo = 0, hi = B;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cu[mid] <= t) lo = mid; else hi = mid;
        }
        int id = ids[t];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        int pos = (t - cu[lo]) + pos_off;
        pos = pos < max_pos ? pos : max_pos - 1;
        const float* wr_ = wemb + (size_t)id * H;
        const float* pr_ = pemb + (size_t)pos * H;
        // seg / tdelta as in k_embed_ln: the type-1 add comes before the bf16 rounding, so the sums stay those of the
        // stored values
        const bool ty1 = seg_type1(seg, lo, t - cu[lo], cu[lo + 1] - cu[lo]);
        char* orow = reinterpret_cast<char*>(pre) + (size_t)(t >> 4) * preblk_rowstride(H) + lq * 16;
#pragma unroll
        for (int pi = g; pi < NP; pi += 16) {
            const int cb = pi >> 3, j = (pi >> 2) & 1, lg = pi & 3;
            const int c0 = 64 * cb + 32 * j + 4 * lg;
            const float4 a0 = *reinterpret_cast<const float4*>(wr_ + c0), a1 = *reinterpret_cast<const float4*>(wr_ + c0 + 16);
            const float4 b0 = *reinterpret_cast<const float4*>(pr_ + c0), b1 = *reinterpret_cast<const float4*>(pr_ + c0 + 16);
            float v[8] = {a0.x + b0.x, a0.y + b0.y, a0.z + b0.z, a0.w + b0.w, a1.x + b1.x, a1.y + b1.y, a1.z + b1.z, a1.w + b1.w};
            if (ty1) {
                const float4 d0 = *reinterpret_cast<const float4*>(tdelta + c0), d1 = *reinterpret_cast<const float4*>(tdelta + c0 + 16);
                v[0] += d0.x; v[1] += d0.y; v[2] += d0.z; v[3] += d0.w;
                v[4] += d1.x; v[5] += d1.y; v[6] += d1.z; v[7] += d1.w;
            }
            unsigned o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bf16_t h0 = f2bf(v[2 * e]), h1 = f2bf(v[2 * e + 1]);
                o[e] = (unsigned)h0 | ((unsigned)h1 << 16);
                const float x = bf2f(h0), y = bf2f(h1);   // statistics of the STORED values
                s1 += x + y;
                s2 += x * x + y * y;
            }
            *reinterpret_cast<uint4*>(orow + (size_t)cb * 2048 + j * 1024 + lg * 256) = uint4{o[0], o[1], o[2], o[3]};
        }
    }
    red[0][g][lq] = s1;
    red[1][g][lq] = s2;
    __syncthreads();
    if (g == 0 && t < T) {   // fixed summation order: a forward pass stays bit reproducible
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            a += red[0][i][lq];
            b += red[1][i][lq];
        }
        stats[(size_t)t * 2] = __float2ll_rn(a * scale1);
        stats[(size_t)t * 2 + 1] = __float2ll_rn(b * scale2);
    }
}

// Weight preparation of the LayerNorm-folded path, one wave per output row j of W [N][K]:
//   Wf[j][k] = bf16(W[j][k] gamma[k] - mean_k(W[j][.] gamma[.])),   d[j] = sum_k beta[k] W[j][k] + bias[j].
__global__ __launch_bounds__(256) void k_fold_ln(const float* __restrict__ W, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ bias,
                                                 int N, int K, bf16_t* __restrict__ Wf, float* __restrict__ dvec, int perm) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N) return;
    float c = 0.f, d = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = W[(size_t)j * K + k];
        c = fmaf(w, gamma[k], c);
        d = fmaf(beta[k], w, d);
    }
    c = wave_allsum(c) / (float)K;
    d = wave_allsum(d);
    // perm: the A operand is a pre tensor in the blocked layout, whose K order inside a 64-column block is permuted
    for (int k = lane; k < K; k += 64)
        Wf[perm ? (G8_BBLK ? preblk_elem(j, k, K) : (size_t)j * K + preblk_kpos(k)) : (size_t)j * K + k] = f2bf(fmaf(W[(size_t)j * K + k], gamma[k], -c));
    if (lane == 0) dvec[j] = d + bias[j];
}

__global__ void k_add_vec(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// LayerNorm of token rows: LN(in + resid) (the GEMM epilogue added the bias; the residual add lives
// here, where the access is perfectly coalesced, so the GEMM epilogue is store-only).  The arithmetic
// is fp32; TPre / TRes are the storage types of the GEMM output and of the residual stream (float, or
// bf16 in the product mode: the residual then is the same bf16 row the next GEMM reads, and the kernel
// moves 6 B per element instead of 14).  out32 may be null (only the last LN of the stack feeds the
// fp32 pooling).
template <typename T>
__device__ __forceinline__ float4 ln_load4(const T* row, int idx);
template <>
__device__ __forceinline__ float4 ln_load4<float>(const float* row, int idx) {
    return reinterpret_cast<const float4*>(row)[idx];
}
template <>
__device__ __forceinline__ float4 ln_load4<bf16_t>(const bf16_t* row, int idx) {
    const ushort4 h = reinterpret_cast<const ushort4*>(row)[idx];
    return make_float4(__uint_as_float((unsigned)h.x << 16), __uint_as_float((unsigned)h.y << 16),
                       __uint_as_float((unsigned)h.z << 16), __uint_as_float((unsigned)h.w << 16));
}

template <int H, typename TPre, typename TRes>
__global__ __launch_bounds__(256) void k_layernorm(const TPre* __restrict__ in, const TRes* __restrict__ resid,
                                                   const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps,
                                                   float* __restrict__ out32, bf16_t* __restrict__ out16, int T) {
    static_assert(H % 128 == 0, "float4 columns of a row cover whole 32-lane halves");
    constexpr int NV = (H / 4 + 63) / 64;   // (k_embed_ln: the lanes beyond H / 4 of the last round idle)
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const TPre* xrow = in + (size_t)t * H;
    const TRes* rrow = resid + (size_t)t * H;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float4 a = ln_load4<TPre>(xrow, lane + 64 * i), b = ln_load4<TRes>(rrow, lane + 64 * i);
        v[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_allsum(s) * (1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = rsqrtf(wave_allsum(q) * (1.0f / H) + eps);
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float4 g = g4[lane + 64 * i], b = b4[lane + 64 * i];
        float4 o;
        o.x = (v[i].x - mean) * rstd * g.x + b.x;
        o.y = (v[i].y - mean) * rstd * g.y + b.y;
        o.z = (v[i].z - mean) * rstd * g.z + b.z;
        o.w = (v[i].w - mean) * rstd * g.w + b.w;
        if (out32) reinterpret_cast<float4*>(out32 + (size_t)t * H)[lane + 64 * i] = o;
        if (out16) {
            ushort4 h;
            h.x = f2bf(o.x); h.y = f2bf(o.y); h.z = f2bf(o.z); h.w = f2bf(o.w);
            reinterpret_cast<ushort4*>(out16 + (size_t)t * H)[lane + 64 * i] = h;
        }
    }
}

// ---------------------------------------------------------------- GEMM
// C[M,N] = A[M,K] * W[N,K]^T (+ epilogue).  Both operands are K-contiguous, so A
// and W fragments are 16-B rows-of-K vectors.  Block = WM x WN waves, each wave a
// (32*TM) x (32*TN) output tile; a ring stage holds RB bytes of K per row.
//
// Staging is LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave instruction) into a ring of NST
// stages with COUNTED vmcnt and a raw s_barrier.  The product configuration is 2 stages x 64 KiB
// (256 + 256 rows x 128 B): measured on MI355X, a CU takes ~45-49 GB/s into LDS whatever the
// number of stages in flight (a bandwidth limit), and rings of 3-5 smaller stages only added
// barriers.  The 128x128 configuration (small shapes) keeps a 4 x 16 KiB ring of 64-B rows.
// LDS rows of 128 B: physical 16-B chunk = logical ^ ((row>>1)&7); rows of 64 B: logical ^
// ((row>>2)&3): every ds_read_b128 lane group hits 16 distinct slots.  The swizzle is applied
// on the per-lane SOURCE address of the DMA (its LDS destination is linear) and on reads.
// k_gemm16 (below) is the product-mode twin of the 256x256 bf16 configuration on 16x16x32 MFMAs.
enum { EPI_QKV = 0, EPI_GELU = 1, EPI_RESID = 2,
       // k_gemm8p only: LayerNorm folded into the GEMMs (see "LayerNorm without LayerNorm kernels" below)
       EPI_AFF_QKV = 3, EPI_AFF_GELU = 4, EPI_RES = 5 };

template <typename TIn>
struct GemmTraits;
template <>
struct GemmTraits<bf16_t> {};
template <>
struct GemmTraits<float> {};

__device__ __forceinline__ int swz64_byte(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// erf by Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7): two transcendentals + ~10 VALU
// instead of erff's ~40; used where the result is rounded to bf16 anyway.
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));  // v_rcp_f32 (1 ulp); __frcp_rn expands to the full IEEE division sequence
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.0f - p * t * __expf(-z * z);
    return 0.5f * x * (1.0f + copysignf(e, x));
}

// GELU without transcendentals (the product GEMM's epilogue is VALU bound: v_rcp / v_exp issue at a quarter of the
// plain rate and were 40 % of gelu_erf_fast's cycles).  gelu(x) = x Phi(x), Phi(x) = 1/2 + x E(x^2) with
// E(s) = erf(sqrt(s/2)) / (2 sqrt(s)), an entire function of s: a degree-8 polynomial in s on [0, 4.25^2] (weighted
// minimax fit of s E(s), constrained to E(4.25^2) = 1 / (2 * 4.25) so that Phi(+-4.25) is exactly 1 / 0), evaluated
// at xc = clamp(x, -4.25, 4.25): beyond the clamp Phi stays 1 / 0, i.e. gelu = x / 0 (|gelu(-4.25)| = 4.5e-5).
// |error| <= 6e-5 absolute against erf GELU in fp32 Horner form (checked over [-9, 9] in 1e-5 steps; 4.5e-5 of it is
// the fit), relative error <= 1e-5 for x > 4.25: below a bf16 half ulp for every |gelu(x)| > 0.03, and the result is
// rounded to bf16 right after.  Per element: one v_med3 + 11 packed-fp32 operations (v_pk_mul / v_pk_fma: two
// elements per instruction) = 6.5 issue slots; the round-1 form (degree 10 in |x| plus integer clamp / relu, scalar
// FMAs) took 15 and was 1.3 ms of the 256x384 forward.
__device__ __forceinline__ v4f gelu_poly4(v4f x) {
    constexpr float A = 4.25f;
    v4f xc;
#pragma unroll
    for (int e = 0; e < 4; ++e) xc[e] = __builtin_amdgcn_fmed3f(x[e], -A, A);
    const v4f s = xc * xc;
#define CSS_GP_C(C_) v4f{C_, C_, C_, C_}
    v4f p = CSS_GP_C(6.7378984336397e-11f);
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(-6.313554568038171e-09f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(2.6018219045909063e-07f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(-6.285347353696125e-06f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(1.00753313745372e-04f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(-1.1566871544346213e-03f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(9.993435814976692e-03f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(-6.666824966669083e-02f));
    p = __builtin_elementwise_fma(p, s, CSS_GP_C(3.9911165833473206e-01f));
    const v4f phi = __builtin_elementwise_fma(xc, p, CSS_GP_C(0.5f));
#undef CSS_GP_C
    return x * phi;
}

// TIn: operand type (bf16_t or float).  Output: EPI_RESID -> fp32 [M,N] = acc + bias (the
// residual is added by k_layernorm); EPI_QKV / EPI_GELU -> TIn [M,N]; EPI_QKV scales columns
// < qscale_cols by 0.125 (1/sqrt(64)).
//
// PERSISTENT: one block per CU walks its share of the output tiles; the LDS-DMA ring runs
// 3 stages ahead ACROSS tile boundaries (no per-tile pipeline fill), and a tile's epilogue
// is store-only (bias comes from LDS), so its stores drain underneath the next tile's MFMAs.
// vmcnt bookkeeping is exact: the only vector-memory operations in the steady state are
// PPW LDS-DMA instructions per stage and E unconditional stores per tile (rows beyond M land
// in the slack rows every activation buffer has).
template <typename TIn, int EPI, int WM, int WN, int TM, int TN, int NST, int RB, int SPS>
__global__ __launch_bounds__(WM* WN * 64) void k_gemm(const TIn* __restrict__ A, const TIn* __restrict__ W,
                                                      const float* __restrict__ bias, void* __restrict__ Cout, int M,
                                                      int N, int K, int qscale_cols, float qscale) {
    static_assert(RB == 64 || RB == 128, "stage rows are 64 or 128 bytes of K");
    constexpr int BK = RB / (int)sizeof(TIn);  // K elements per stage
    constexpr bool BF = sizeof(TIn) == 2;
    constexpr int NW = WM * WN;
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    constexpr int A_BYTES = BM * RB, B_BYTES = BN * RB, STAGE = A_BYTES + B_BYTES;
    constexpr int RPP = 1024 / RB;             // rows per 1-KiB LDS-DMA piece (16 or 8)
    constexpr int CPR = RB / 16;               // 16-B chunks per row (4 or 8)
    constexpr int PIECES = (BM + BN) / RPP;    // 1-KiB LDS-DMA pieces per stage
    static_assert(PIECES % NW == 0, "pieces must divide over the waves");
    constexpr int PPW = PIECES / NW;        // LDS-DMA instructions per wave per stage
    constexpr bool OUT16 = BF && EPI == EPI_QKV;  // these bf16 outputs leave as 16-B stores (2 per 32x32 block)
    constexpr int E = TM * TN * (OUT16 ? 2 : 4);  // store instructions per wave per tile (vmcnt bookkeeping)
    // SPS ring stages are consumed per barrier step; Y stages stay in flight across a step's wait
    constexpr int Y = NST - 2 * SPS;
    static_assert(Y >= 0 && Y <= 2 && (SPS == 1 || SPS == 2), "ring shape");
    static_assert(Y * PPW + E <= 63, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [NST][A_BYTES | B_BYTES]
    // The tile's BN bias values travel global -> registers of wave 0 (second step of the tile) -> this static
    // LDS array (third step) -> 16-B epilogue reads.  (256 scalar loads per tile, each pinned and waited for, used
    // to cost 8-15 us per tile: more than a third of a K = 768 tile; a copy inside the dynamic ring made hipcc
    // drain the DMA queue before reading it, a separate LDS object does not alias the ring.)
    __shared__ __attribute__((aligned(16))) float sbias[BN];
    static_assert(BN <= 256, "one wave stages the bias row of a tile");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WN, wc = wave % WN;
    float4 bias_regs = make_float4(0.f, 0.f, 0.f, 0.f);
    const int fr = lane & 31, fh = lane >> 5;

    // XCD-aware persistent tile walk: XCD x (blocks with blockIdx % 8 == x under round-robin
    // dispatch; speed only) owns a contiguous range of tiles in N-fastest order and its blocks
    // advance through it side by side, so neighbouring blocks share A row panels in one L2.
    const int ntn = N / BN, ntm = (M + BM - 1) / BM;
    const int nwg = ntn * ntm;
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3, per_x = gridDim.x >> 3;
    const int q = nwg / 8, r = nwg % 8;
    const int xfirst = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int xcount = q + (xcd < r ? 1 : 0);
    const int my_ntiles = jx < xcount ? (xcount - jx + per_x - 1) / per_x : 0;
    const int KT = K / BK;
    const int total = my_ntiles * KT;
    if (total == 0) return;

    const int prow = lane / CPR, pchunk = lane % CPR;
    const char* src[PPW];  // issue-side per-lane source pointers (current issue tile)
    int dst[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int piece = wave + NW * i;
        const bool isA = piece < BM / RPP;
        dst[i] = (isA ? 0 : A_BYTES) + (isA ? piece : piece - BM / RPP) * 1024;
    }
    auto set_src = [&](int tile_idx) {
        const int tile = xfirst + jx + tile_idx * per_x;
        const int r0 = (tile / ntn) * BM, c0 = (tile % ntn) * BN;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int piece = wave + NW * i;
            const bool isA = piece < BM / RPP;
            const int trow = (isA ? piece : piece - BM / RPP) * RPP + prow;
            const int logical = RB == 64 ? (pchunk ^ ((trow >> 2) & 3)) : (pchunk ^ ((trow >> 1) & 7));
            int grow = (isA ? r0 : c0) + trow;
            const int lim = isA ? M : N;
            grow = grow < lim ? grow : lim - 1;
            src[i] = reinterpret_cast<const char*>((isA ? A : W) + (size_t)grow * K) + logical * 16;
        }
    };
#define GM_ISSUE(KT_, SLOT_)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < PPW; ++i) {                                                        \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[i] + (size_t)(KT_) * RB), \
                                         (__attribute__((address_space(3))) void*)(smem + (SLOT_) * STAGE + dst[i]), 16, 0, 0); \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) acc[m][n][r2] = 0.f;

    // issue side runs NST-SPS stages ahead of the compute side
    int it_tile = 0, it_kt = 0, gi = 0;  // gi: global stage index of the next stage to issue
    set_src(0);
    for (int p = 0; p < NST - SPS && gi < total; ++p) {
        GM_ISSUE(it_kt, gi % NST)
        ++gi;
        if (++it_kt == KT) {
            it_kt = 0;
            if (++it_tile < my_ntiles) set_src(it_tile);
        }
    }
    int ct_tile = 0, kt = 0;
    for (int g = 0; g < total; g += SPS) {  // total and KT are multiples of SPS (host check)
        // stages g .. g+SPS-1 have landed once only the younger operations are outstanding
        const int younger = min(Y, total - 1 - (g + SPS - 1));  // stages issued after them, allowed in flight
        // this tile's first NST-SPS stages were issued before the previous tile's epilogue stores
        const bool stores_younger = ct_tile > 0 && (kt + SPS - 1) < NST - SPS;
        if (stores_younger) {
            // (KT >= NST: the Y younger stages exist here)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Y * PPW + E) : "memory");
        } else if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((Y >= 2 ? 2 : 0) * PPW) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((Y >= 1 ? 1 : 0) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wave == 0 && kt == 2 * SPS) {  // bias row of this tile -> LDS (visible after this step's barrier)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane < BN / 4) *reinterpret_cast<float4*>(&sbias[4 * lane]) = bias_regs;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();  // all pieces of this step's stages landed; the previous step's slots are free
        if (wave == 0 && kt == SPS && lane < BN / 4) {
            const int tile_b = xfirst + jx + ct_tile * per_x;
            bias_regs = *reinterpret_cast<const float4*>(bias + (tile_b % ntn) * BN + 4 * lane);
        }
#pragma unroll
        for (int u = 0; u < SPS; ++u)
            if (gi < total) {
                GM_ISSUE(it_kt, gi % NST)
                ++gi;
                if (++it_kt == KT) {
                    it_kt = 0;
                    if (++it_tile < my_ntiles) set_src(it_tile);
                }
            }
#pragma unroll
        for (int u = 0; u < SPS; ++u) {
            const char* Ab = smem + ((g + u) % NST) * STAGE;
            const char* Bb = Ab + A_BYTES;
#pragma unroll
            for (int c = 0; c < CPR / 2; ++c) {
                v4f a[TM], b[TN];
#pragma unroll
                for (int m = 0; m < TM; ++m)
                    a[m] = *reinterpret_cast<const v4f*>(Ab + (RB == 64 ? swz64_byte(wr * (TM * 32) + 32 * m + fr, 2 * c + fh)
                                                                       : swz_byte(wr * (TM * 32) + 32 * m + fr, 2 * c + fh)));
#pragma unroll
                for (int n = 0; n < TN; ++n)
                    b[n] = *reinterpret_cast<const v4f*>(Bb + (RB == 64 ? swz64_byte(wc * (TN * 32) + 32 * n + fr, 2 * c + fh)
                                                                       : swz_byte(wc * (TN * 32) + 32 * n + fr, 2 * c + fh)));
#pragma unroll
                for (int m = 0; m < TM; ++m)
#pragma unroll
                    for (int n = 0; n < TN; ++n) {
                        // transposed product: MFMA rows <- W rows (output columns), MFMA columns <-
                        // tokens.  Each lane then owns ONE output row (token) and 4 consecutive
                        // output columns per register group: 16-B (fp32) / 8-B (bf16) epilogue stores.
                        if constexpr (BF) {
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, b[n]),
                                                                                __builtin_bit_cast(v8bf, a[m]), acc[m][n], 0, 0, 0);
                        } else {
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[n].x, a[m].x, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[n].y, a[m].y, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[n].z, a[m].z, acc[m][n], 0, 0, 0);
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[n].w, a[m].w, acc[m][n], 0, 0, 0);
                        }
                    }
            }
        }
        kt += SPS;
        if (kt == KT) {
            // ---- epilogue of tile ct_tile: bias (LDS) + activation + E unconditional stores.
            // lane = token row (fr of the 32-row tile); register group g4 = the 4 consecutive
            // output columns 8*g4 + 4*fh + {0..3} of each 32-column tile.
            const int tile = xfirst + jx + ct_tile * per_x;
            const int row0 = (tile / ntn) * BM, col0 = (tile % ntn) * BN;
            const int cbase = col0 + wc * (TN * 32) + 4 * fh;
#pragma unroll
            for (int m = 0; m < TM; ++m) {
                const size_t rbase = (size_t)(row0 + wr * (TM * 32) + 32 * m + fr) * N + cbase;  // may be a slack row
#pragma unroll
                for (int n = 0; n < TN; ++n) {
                    uint2 packed[4];  // bf16 outputs: 4 columns per register group, packed 2 per dword
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const int col = cbase + 32 * n + 8 * g4;
                        const float4 bv = *reinterpret_cast<const float4*>(&sbias[wc * (TN * 32) + 32 * n + 8 * g4 + 4 * fh]);
                        float4 v;
                        v.x = acc[m][n][4 * g4 + 0] + bv.x;
                        v.y = acc[m][n][4 * g4 + 1] + bv.y;
                        v.z = acc[m][n][4 * g4 + 2] + bv.z;
                        v.w = acc[m][n][4 * g4 + 3] + bv.w;
                        if constexpr (EPI == EPI_GELU) {
                            if constexpr (BF) {
                                v.x = gelu_erf_fast(v.x); v.y = gelu_erf_fast(v.y); v.z = gelu_erf_fast(v.z); v.w = gelu_erf_fast(v.w);
                            } else {
                                v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w);
                            }
                        }
                        if constexpr (EPI == EPI_QKV) {
                            const float sc = col < qscale_cols ? qscale : 1.0f;  // qscale_cols is a multiple of 4
                            v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
                        }
                        if constexpr (EPI == EPI_RESID || !BF) {
                            *reinterpret_cast<float4*>(reinterpret_cast<float*>(Cout) + rbase + 32 * n + 8 * g4) = v;
                        } else if constexpr (OUT16) {
                            packed[g4].x = (unsigned)f2bf(v.x) | ((unsigned)f2bf(v.y) << 16);
                            packed[g4].y = (unsigned)f2bf(v.z) | ((unsigned)f2bf(v.w) << 16);
                        } else {
                            ushort4 h;
                            h.x = f2bf(v.x); h.y = f2bf(v.y); h.z = f2bf(v.z); h.w = f2bf(v.w);
                            *reinterpret_cast<ushort4*>(reinterpret_cast<bf16_t*>(Cout) + rbase + 32 * n + 8 * g4) = h;
                        }
                    }
                    if constexpr (OUT16) {
                        // A lane holds columns 8 g4 + 4 fh + {0..3}; its partner (lane ^ 32) the other half of each
                        // 8-column group.  Swap halves so that every lane stores 16 B (8 consecutive bf16): row-per-
                        // lane 8-B stores are store-issue bound (MI355X_MICROARCH.md), 16-B stores halve the count.
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            // (v_permlane32_swap_b32 does this exchange without the LDS crossbar; measured 1 % slower)
                            const uint2 mine_a = packed[2 * j], mine_b = packed[2 * j + 1];
                            const uint2 send = fh ? mine_a : mine_b;
                            uint2 recv;
                            recv.x = (unsigned)__shfl_xor((int)send.x, 32);
                            recv.y = (unsigned)__shfl_xor((int)send.y, 32);
                            // fh = 0 stores columns 16 j + 0..7 of the 32-column tile, fh = 1 columns 16 j + 8..15
                            const uint4 o = fh ? make_uint4(recv.x, recv.y, mine_b.x, mine_b.y) : make_uint4(mine_a.x, mine_a.y, recv.x, recv.y);
                            *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(Cout) + rbase - 4 * fh + 32 * n + 16 * j + 8 * fh) = o;
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < TM; ++m)
#pragma unroll
                for (int n = 0; n < TN; ++n)
#pragma unroll
                    for (int r2 = 0; r2 < 16; ++r2) acc[m][n][r2] = 0.f;
            kt = 0;
            ++ct_tile;
        }
    }
#undef GM_ISSUE
}

// ---------------------------------------------------------------- bf16 GEMM on v_mfma_f32_16x16x32_bf16
// The product-mode configuration of k_gemm (bf16, 256x256 tile, 2x4 waves, 2 x 64-KiB LDS-DMA ring) with the
// 16x16x32 MFMA: same cycles per flop and the same LDS traffic as 32x32x16, but the chip holds a higher clock
// under it (MI355X_MICROARCH.md, DVFS item 7; measured +8 % on the kNN scan's identical main loop).
// Accumulator geometry: lane (lq = lane & 15, lg = lane >> 4) holds token row 16 m + lq (m < 8) and the 4
// consecutive output columns 16 n + 4 lg + {0..3} (n < 4) of the wave's 128 x 64 block.
// (Tile-count tails -- N = 768 gives 4.5 tiles per CU -- were tried as 128-token half tiles in the last round:
// no gain, a half tile still moves 3/4 of the stage bytes and the loop is fill bound.)
template <int EPI>
__global__ __launch_bounds__(512) void k_gemm16(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                const float* __restrict__ bias, void* __restrict__ Cout, int M, int N,
                                                int K, int qscale_cols, float qscale) {
    constexpr int NW = 8, WN = 4, TM = 8, TN = 4, BM = 256, BN = 256, RB = 128;
    constexpr int A_BYTES = BM * RB, STAGE = (BM + BN) * RB, PPW = 8;
    static_assert(EPI == EPI_QKV || EPI == EPI_GELU, "bf16 output epilogues");
    constexpr int E = 2 * TM;                         // store instructions per wave per tile (vmcnt bookkeeping)
    static_assert(E <= 63, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][A_BYTES | B_BYTES]
    __shared__ __attribute__((aligned(16))) float sbias[BN];
    // bf16 outputs leave through a per-wave LDS transpose (16 token rows x 64 columns at a time): a lane owns 4
    // columns of one row, so direct stores scatter 8-B pieces over 64 rows per instruction (one L2 transaction
    // each: ~4-8 us per tile); after the transpose 8 lanes write one full 128-B line.  Rows are padded to 144 B
    // (16 rows fall on 16 different bank groups).
    constexpr int EPI_ROW = 144;
    __shared__ __attribute__((aligned(16))) char sepi[NW][16 * EPI_ROW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WN, wc = wave % WN;
    const int lq = lane & 15, lg = lane >> 4;
    float4 bias_regs = make_float4(0.f, 0.f, 0.f, 0.f);

    const int ntn = N / BN, ntm = (M + BM - 1) / BM;
    const int nwg = ntn * ntm;
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3, per_x = gridDim.x >> 3;
    const int q = nwg / 8, r = nwg % 8;
    const int xfirst = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int xcount = q + (xcd < r ? 1 : 0);
    const int my_ntiles = jx < xcount ? (xcount - jx + per_x - 1) / per_x : 0;
    const int KT = K / 64;
    const int total = my_ntiles * KT;
    if (total == 0) return;

    const int prow = lane >> 3, pchunk = lane & 7;
    const char* src[PPW];
    int dst[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int piece = wave + NW * i;
        dst[i] = (piece < 32 ? 0 : A_BYTES) + (piece & 31) * 1024;
    }
    auto set_src = [&](int tile_idx) {
        const int tile = xfirst + jx + tile_idx * per_x;
        const int r0 = (tile / ntn) * BM, c0 = (tile % ntn) * BN;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int piece = wave + NW * i;
            const bool isA = piece < 32;
            const int trow = (piece & 31) * 8 + prow;
            int grow = (isA ? r0 : c0) + trow;
            const int lim = isA ? M : N;
            grow = grow < lim ? grow : lim - 1;
            src[i] = reinterpret_cast<const char*>((isA ? A : W) + (size_t)grow * K) + ((pchunk ^ ((trow >> 1) & 7)) << 4);
        }
    };
#define G16_ISSUE(KT_, SLOT_)                                                                                \
    _Pragma("unroll") for (int i = 0; i < PPW; ++i) {                                                        \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[i] + (size_t)(KT_) * RB), \
                                         (__attribute__((address_space(3))) void*)(smem + (SLOT_) * STAGE + dst[i]), 16, 0, 0); \
    }

    v4f acc[TM][TN];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc[m][n] = v4f{0.f, 0.f, 0.f, 0.f};

    int it_tile = 0, it_kt = 0, gi = 0;
    set_src(0);
    G16_ISSUE(0, 0)
    gi = 1;
    if (++it_kt == KT) {
        it_kt = 0;
        if (++it_tile < my_ntiles) set_src(it_tile);
    }
    int ct_tile = 0, kt = 0;
    for (int g = 0; g < total; ++g) {
        // the tile's first stage was issued before the previous tile's E epilogue stores
        if (ct_tile > 0 && kt == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(E) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (wave == 0 && kt == 2) {  // bias row of this tile -> LDS (visible after this step's barrier)
            *reinterpret_cast<float4*>(&sbias[4 * lane]) = bias_regs;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (wave == 0 && kt == 1) {
            const int tile_b = xfirst + jx + ct_tile * per_x;
            bias_regs = *reinterpret_cast<const float4*>(bias + (tile_b % ntn) * BN + 4 * lane);
        }
        if (gi < total) {
            G16_ISSUE(it_kt, gi & 1)
            ++gi;
            if (++it_kt == KT) {
                it_kt = 0;
                if (++it_tile < my_ntiles) set_src(it_tile);
            }
        }
        const char* Ab = smem + (g & 1) * STAGE;
        const char* Bb = Ab + A_BYTES;
#pragma unroll
        for (int c = 0; c < 2; ++c) {  // two 32-wide k steps per 64-wide stage
            v4f a[TM], b[TN];
#pragma unroll
            for (int m = 0; m < TM; ++m) a[m] = *reinterpret_cast<const v4f*>(Ab + swz_byte(wr * 128 + 16 * m + lq, 4 * c + lg));
#pragma unroll
            for (int n = 0; n < TN; ++n) b[n] = *reinterpret_cast<const v4f*>(Bb + swz_byte(wc * 64 + 16 * n + lq, 4 * c + lg));
#pragma unroll
            for (int m = 0; m < TM; ++m)
#pragma unroll
                for (int n = 0; n < TN; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, b[n]),
                                                                        __builtin_bit_cast(v8bf, a[m]), acc[m][n], 0, 0, 0);
        }
        if (++kt == KT) {
            const int tile = xfirst + jx + ct_tile * per_x;
            const int col0 = (tile % ntn) * BN + wc * 64;
            float4 bv[TN];
#pragma unroll
            for (int n = 0; n < TN; ++n) bv[n] = *reinterpret_cast<const float4*>(&sbias[wc * 64 + 16 * n + 4 * lg]);
#pragma unroll
            for (int m = 0; m < TM; ++m) {
                char* mine = sepi[wave];
#pragma unroll
                for (int n = 0; n < TN; ++n) {
                    float4 v;
                    v.x = acc[m][n][0] + bv[n].x;
                    v.y = acc[m][n][1] + bv[n].y;
                    v.z = acc[m][n][2] + bv[n].z;
                    v.w = acc[m][n][3] + bv[n].w;
                    if constexpr (EPI == EPI_GELU) {
                        v.x = gelu_erf_fast(v.x); v.y = gelu_erf_fast(v.y); v.z = gelu_erf_fast(v.z); v.w = gelu_erf_fast(v.w);
                    }
                    if constexpr (EPI == EPI_QKV) {
                        const float sc = col0 + 16 * n < qscale_cols ? qscale : 1.0f;  // qscale_cols is a multiple of 16
                        v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
                    }
                    uint2 pk;
                    pk.x = (unsigned)f2bf(v.x) | ((unsigned)f2bf(v.y) << 16);
                    pk.y = (unsigned)f2bf(v.z) | ((unsigned)f2bf(v.w) << 16);
                    *reinterpret_cast<uint2*>(mine + lq * EPI_ROW + (16 * n + 4 * lg) * 2) = pk;
                }
                // read the 16 x 64 block back row-wise: lane j -> row 8 t + (j >> 3), 16-B chunk j & 7
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int rr = 8 * t + (lane >> 3);
                    const uint4 o = *reinterpret_cast<const uint4*>(mine + rr * EPI_ROW + (lane & 7) * 16);
                    const size_t g = (size_t)((tile / ntn) * BM + wr * 128 + 16 * m + rr) * N + col0 + (lane & 7) * 8;
                    *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(Cout) + g) = o;
                }
            }
#pragma unroll
            for (int m = 0; m < TM; ++m)
#pragma unroll
                for (int n = 0; n < TN; ++n) acc[m][n] = v4f{0.f, 0.f, 0.f, 0.f};
            kt = 0;
            ++ct_tile;
        }
    }
#undef G16_ISSUE
}

// ---------------------------------------------------------------- bf16 GEMM, 8-phase ping-pong main loop
// The product-mode GEMM of the encoder (same contract as k_gemm16: C[M,N] bf16 = A[M,K] . W[N,K]^T + bias, then the
// EPI transform; 256 x 256 tiles, persistent, XCD-aware tile walk) with the main loop restructured after the
// "256^2 8-phase template" of cdna_hip_programming.md:
//
//   * a 64-deep K step is four PHASES of 16 MFMAs (one quadrant of the wave's 128 x 64 output each); every phase is
//     [fragment reads + 2 LDS-DMA instructions]  s_barrier  [16 MFMAs]  s_barrier;
//   * wave row 1 (waves 4..7) runs ONE barrier behind wave row 0, so on every SIMD one wave issues MFMAs while its
//     partner reads fragments and issues DMA (MI355X_MICROARCH.md, "Two waves per SIMD", item 9);
//   * LDS = 2 K-step buffers x 4 half-tile slots of 16 KiB, in issue order A0, B0, B1, A1:
//         A_s: rows {wr*128 + s*64 + [0,64)}, slot row wr*64 + r   (a wave row reads and refills only its own 64 rows)
//         B_s: rows {wc*64 + s*32 + [0,32)},  slot row wc*32 + r
//     K step u (buffer D = u & 1):  P1 reads A_0, B_0   issues A_1(u+1) -> D^1      MFMA (A0, B0)
//                                   P2 reads B_1        issues A_0(u+2) -> D        MFMA (A0, B1)
//                                   P3 reads A_1        issues B_0(u+2) -> D        MFMA (A1, B1)
//                                   P4 (B_0 in regs)    issues B_1(u+2) -> D        MFMA (A1, B0)
//     so three half tiles stay in flight behind a counted vmcnt(6) at P4 (K step u+1 has landed; its first reads
//     come two barriers later).  A slot is refilled one phase after its last read when only the refilling wave
//     row reads it (A), two phases after when both wave rows read it (B): with the one-barrier stagger every read
//     has been waited for (lgkmcnt(0) right behind the phase's first barrier) before the refill is issued;
//   * accumulators START from the bias row (DMA'd into LDS one tile ahead, read with inline-asm ds_read: a
//     compiler-visible LDS read beside pending LDS-DMA makes hipcc drain the queue with vmcnt(0)); the epilogue is
//     EPI transform -> bf16 -> per-wave 16 x 64 LDS transpose (inline asm, same reason) -> 16-B nontemporal stores
//     of full 128-B lines.
// Measured on MI355X (tools/gemm_lab.hip, same data, one process): 98304 x 2304 x 768: 0.300 vs 0.360 ms for
// k_gemm16; x 768 x 768: 0.107 vs 0.134; x 768 x 3072: 0.361 vs 0.457.  Requires K % 128 == 0, N % 256 == 0,
// M * K * 2 < 4 GiB (32-bit source offsets) and >= 256 slack rows behind A and C.
//
// LayerNorm without LayerNorm kernels (EPI_AFF_*, EPI_RES).  The post-LN stack is x = LN(pre) with pre = branch
// output + residual.  The product path never materialises x:
//   * a GEMM that CONSUMES x (QKV, FFN1) reads the un-normalised pre (bf16) with weights folded at load time
//     (k_fold_ln): W'[j,k] = W[j,k] gamma[k] - mean_k(W[j,.] gamma), rows centred so that the mean of the token row
//     drops out (sum_k (pre_k - mu) = 0):   x.W^T + b = rs_t (pre_t . W'_j) + d_j,   d_j = sum_k beta[k] W[j,k] + b_j.
//     The epilogue is one fma per element from the row's rs (EPI_AFF_*).  (bf16 rounding leaves row sums of W' of
//     ~1e-3 instead of 0: an error of mu rs 1e-3 per output, below the bf16 resolution of the outputs for any
//     |mu| of the order of the row's standard deviation.)
//   * a GEMM that PRODUCES a pre (O projection, FFN2) adds bias' = bias + beta and the rest of the residual
//     LN(previous pre) = gamma (p rs - mu rs) + beta, recomputed in the accumulator layout from the previous pre
//     tensor and its row statistics, stores the new pre as bf16 and accumulates the row sums (EPI_RES).
// Row statistics travel as raw (sum, sum^2) pairs [T][2] in 64-bit FIXED POINT (sum * 2^24, sum^2 * 2^20): each
// wave adds the sums of its 64 columns (fp32, fixed order) with an integer atomic, so the totals do not depend on
// the order the waves arrive in and a forward pass stays bit-reproducible.  mu = sum / H, rs = rsqrt(sum^2 / H -
// mu^2 + eps).  The EPI_AFF_* GEMM of a layer zeroes the statistics the following EPI_RES GEMM accumulates into.
// Per tile the side data (bias or d row, c row, 256 row-statistic pairs) is DMA'd into LDS one tile ahead.
// (range: sum^2 * 2^20 fits 63 bits up to a row sum of squares of 8.8e12, i.e. |pre| ~ 1e5 on all 768 columns; MPNet's
// pre-LayerNorm activations are below 1e3.  Beyond it the conversion saturates and the row's statistics are wrong.)
constexpr float kStatScale1 = 16777216.f, kStatScale2 = 1048576.f;
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void row_stats_decode(v4u32 raw, float inv_h, float eps, float& rs, float& mrs) {
    // int64 -> float as hi * 2^32 + lo (two conversions and an fma; the compiler's exact sequence is ~4x longer)
    const float s1 = fmaf((float)(int)raw[1], 4294967296.f, (float)raw[0]);
    const float s2 = fmaf((float)(int)raw[3], 4294967296.f, (float)raw[2]);
    const float mu = s1 * (1.0f / kStatScale1) * inv_h;
    const float var = fmaf(s2 * (1.0f / kStatScale2), inv_h, -mu * mu);
    rs = rsqrtf(fmaxf(var, 0.f) + eps);
    mrs = mu * rs;
}
struct G8Side {
    const long long* stats_in;   // [T][2] raw row sums of the GEMM's input pre (AFF) / of the residual's pre (RES)
    const float* cvec;       // [N]    RES: gamma of the LayerNorm that makes the residual (its beta is in `bias`)
    const bf16_t* pprev;     // [T][N] RES: the pre whose LayerNorm is the residual
    long long* stats_out;    // [T][2] RES: row sums of the pre written by this GEMM; AFF: zeroed for the next EPI_RES GEMM
    float inv_h;             // 1 / hidden
    float eps;
};

constexpr int G8_HT = 16384;
constexpr int G8_A0 = 0, G8_B0 = 1, G8_B1 = 2, G8_A1 = 3;

// `bias`: the bias row (EPI_QKV / EPI_GELU), bias + beta of the residual's LayerNorm (EPI_RES) or the d row (EPI_AFF_*)
// ABLK: the A operand is in the blocked layout (a pre tensor, or the FFN1 output read by FFN2); the output is written
// in the blocked layout by EPI_RES (pre tensors) and EPI_AFF_GELU (the FFN1 output, whose only reader is FFN2's A side).
// TAG only names the instantiation (rocprofv3 then lists the O projection, <EPI_RES, true, 1>, apart from FFN2, <EPI_RES, true, 0>).
template <int EPI, bool ABLK, int TAG = 0>
__global__ __launch_bounds__(512) void k_gemm8p(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                const float* __restrict__ bias, bf16_t* __restrict__ Cout, int M, int N,
                                                int K, int qscale_cols, float qscale, G8Side side) {
    static_assert(EPI == EPI_QKV || EPI == EPI_GELU || EPI == EPI_AFF_QKV || EPI == EPI_AFF_GELU || EPI == EPI_RES,
                  "bf16 output epilogues");
    constexpr bool AFF = EPI == EPI_AFF_QKV || EPI == EPI_AFF_GELU;
    constexpr bool RES = EPI == EPI_RES;
    constexpr bool DO_GELU = EPI == EPI_GELU || EPI == EPI_AFF_GELU;
    constexpr bool DO_QSCALE = EPI == EPI_QKV || EPI == EPI_AFF_QKV;
    constexpr bool OBLK = RES || AFF;   // output in the blocked layout (preblk_elem): no LDS transpose in the epilogue
    constexpr int NW = 8, BM = 256, BN = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][4][G8_HT]
    // side data of two tiles (parity): [0] bias / d row, [1] gamma row (RES), [2..5] 256 (sum, sum^2) pairs of 16 B
    __shared__ __attribute__((aligned(16))) float sbias[2][6][BN];
    constexpr int EPI_ROW = 144;
    __shared__ __attribute__((aligned(16))) char sepi[NW][16 * EPI_ROW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int lq = lane & 15, lg = lane >> 4;

    const int ntn = N / BN, ntm = (M + BM - 1) / BM;
    const int nwg = ntn * ntm;
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3, per_x = gridDim.x >> 3;
    const int q = nwg / 8, r = nwg % 8;
    const int xfirst = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int xcount = q + (xcd < r ? 1 : 0);
    const int my_ntiles = jx < xcount ? (xcount - jx + per_x - 1) / per_x : 0;
    const int KT = K / 64;                 // even (host check)
    const int total = my_ntiles * KT;      // K steps of this block
    if (total == 0) return;
    // Tile walk inside the XCD's range: N-fastest, so the 32 blocks of an XCD work side by side on a few row panels x
    // ALL tile columns.
#define G8_TILE(IDX_) (xfirst + (IDX_))

    // ---- DMA bookkeeping: one 32-bit source offset per half-tile kind (its first 1-KiB piece; the second piece is 8
    // rows further and its swizzled chunk differs by XOR 4), advanced independently.  Rows beyond M read the slack
    // rows of the activation buffer (their outputs land in slack rows too).
    const int prow = lane >> 3, pchunk = lane & 7;
    unsigned srco[4];
    int it_tile[4], it_kt[4];
    int dsto[4];  // byte offset of this wave's first piece inside a slot
    dsto[G8_A0] = dsto[G8_A1] = (wr * 64 + wc * 16) * 128;
    dsto[G8_B0] = dsto[G8_B1] = (16 * wave) * 128;
    const unsigned row8 = 8u * (unsigned)K * 2u;
#define G8_SET_SRC(KIND_)                                                                                     \
    {                                                                                                         \
        const int tile_ = G8_TILE(jx + it_tile[KIND_] * per_x);                                               \
        const int r0_ = (tile_ / ntn) * BM, c0_ = (tile_ % ntn) * BN;                                         \
        int srow_, grow_;                                                                                     \
        if ((KIND_) == G8_A0 || (KIND_) == G8_A1) {                                                           \
            const int rr_ = wc * 16 + prow;                                                                   \
            srow_ = wr * 64 + rr_;                                                                            \
            grow_ = r0_ + wr * 128 + ((KIND_) == G8_A1 ? 64 : 0) + rr_;                                       \
        } else {                                                                                              \
            srow_ = 16 * wave + prow;                                                                         \
            grow_ = c0_ + (srow_ >> 5) * 64 + ((KIND_) == G8_B1 ? 32 : 0) + (srow_ & 31);                     \
        }                                                                                                     \
        if (ABLK && ((KIND_) == G8_A0 || (KIND_) == G8_A1)) {                                                 \
            /* blocked pre tensor: this wave's 16 rows are ONE 16-row block; its 2 KiB at K step u are copied as they */ \
            /* stand (two 1-KiB pieces, source and LDS destination both contiguous): lane = piece (lg, lq) of half j  */ \
            srco[KIND_] = (unsigned)((r0_ + wr * 128 + ((KIND_) == G8_A1 ? 64 : 0) + wc * 16) >> 4) * (unsigned)preblk_rowstride(K) + \
                          (unsigned)lane * 16u;                                                               \
        } else if (ABLK && G8_BBLK) {   /* weights stored blocked as well (preblk_elem over [N][K]): wave w copies block row */ \
            srco[KIND_] = (unsigned)((c0_ + (wave >> 1) * 64 + ((KIND_) == G8_B1 ? 32 : 0) + 16 * (wave & 1)) >> 4) * \
                          (unsigned)preblk_rowstride(K) + (unsigned)lane * 16u;                               \
        } else {                                                                                              \
            srco[KIND_] = (unsigned)grow_ * (unsigned)K * 2u + ((pchunk ^ ((srow_ >> 1) & 7)) << 4);          \
        }                                                                                                     \
    }
// issue kind KIND_ of its next K step into buffer DB_, then advance that kind's cursor (past the block's last K
// step the cursor keeps re-reading the last tile: harmless -- the slot it lands in is never read again -- and it
// keeps the issue free of branches)
#define G8_ISSUE(KIND_, DB_)                                                                                  \
    {                                                                                                         \
        const char* base_ = reinterpret_cast<const char*>(((KIND_) == G8_A0 || (KIND_) == G8_A1) ? A : W);    \
        const bool ablk_ = ABLK && (G8_BBLK || (KIND_) == G8_A0 || (KIND_) == G8_A1);   /* (blocked: K step = next 2-KiB block, half j = 1 follows) */ \
        const unsigned o0_ = srco[KIND_] + (unsigned)it_kt[KIND_] * (ablk_ ? 2048u : 128u);                   \
        const unsigned o1_ = ablk_ ? (o0_ + 1024u) : ((o0_ + row8) ^ 64u);                                    \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base_ + o0_),        \
            (__attribute__((address_space(3))) void*)(smem + ((DB_) * 4 + (KIND_)) * G8_HT + dsto[KIND_]), 16, 0, 0); \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base_ + o1_),        \
            (__attribute__((address_space(3))) void*)(smem + ((DB_) * 4 + (KIND_)) * G8_HT + dsto[KIND_] + 1024), 16, 0, 0); \
        if (++it_kt[KIND_] == KT) {                                                                           \
            it_kt[KIND_] = 0;                                                                                 \
            if (it_tile[KIND_] + 1 < my_ntiles) {                                                             \
                ++it_tile[KIND_];                                                                             \
                G8_SET_SRC(KIND_)                                                                             \
            }                                                                                                 \
        }                                                                                                     \
    }
// side data of tile TI_ -> sbias[TI_ & 1]: 1-KiB DMA pieces, one per wave (0: bias / d row, 1: gamma row, 2..5: the
// tile's 256 row-statistic pairs)
#define G8_BIAS(TI_)                                                                                          \
    if (wave < ((AFF || RES) ? 6 : 1) && !((AFF) && wave == 1)) {                                             \
        const int tile_b = G8_TILE(jx + (TI_) * per_x);                                                       \
        const float* sp_ = wave == 0 ? bias + (tile_b % ntn) * BN                                             \
                         : (wave == 1 ? side.cvec + (tile_b % ntn) * BN                                       \
                                      : reinterpret_cast<const float*>(side.stats_in + (size_t)(tile_b / ntn) * BM * 2) + (wave - 2) * 256);  \
        __builtin_amdgcn_global_load_lds(                                                                     \
            (const __attribute__((address_space(1))) void*)(sp_ + 4 * lane),                                  \
            (__attribute__((address_space(3))) void*)(&sbias[(TI_) & 1][wave][0]), 16, 0, 0);                  \
    }
// accumulators := bias row PAR_ (inline-asm LDS reads, see the header comment)
#define G8_ACC_FROM_BIAS(PAR_)                                                                                \
    {                                                                                                         \
        v4f bv_[4];                                                                                           \
        const unsigned sboff_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&sbias[PAR_][0][wc * 64 + 4 * lg]; \
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\t" \
                     "ds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"                                 \
                     : "=&v"(bv_[0]), "=&v"(bv_[1]), "=&v"(bv_[2]), "=&v"(bv_[3]) : "v"(sboff_) : "memory");   \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        if constexpr (AFF) { /* zeros, kept opaque so that they are copied with 64-bit moves like the bias */  \
            bv_[0] = v4f{0.f, 0.f, 0.f, 0.f};                                                                 \
            asm volatile("" : "+v"(bv_[0]));                                                                  \
            bv_[1] = bv_[2] = bv_[3] = bv_[0];                                                                \
        }                                                                                                     \
        _Pragma("unroll") for (int m = 0; m < 8; ++m)                                                         \
            _Pragma("unroll") for (int n = 0; n < 4; ++n) acc[m][n] = bv_[n];                                 \
    }
#pragma unroll
    for (int kd = 0; kd < 4; ++kd) {
        it_tile[kd] = 0;
        it_kt[kd] = 0;
    }
    G8_SET_SRC(G8_A0)
    G8_SET_SRC(G8_B0)
    G8_SET_SRC(G8_B1)
    G8_SET_SRC(G8_A1)

    v4f acc[8][4];
    // ---- prologue: K step 0 entirely, K step 1 without its A_1
    G8_BIAS(0)
    G8_ISSUE(G8_A0, 0)
    G8_ISSUE(G8_B0, 0)
    G8_ISSUE(G8_B1, 0)
    G8_ISSUE(G8_A1, 0)
    G8_ISSUE(G8_A0, 1)   // (total >= 2: KT is even)
    G8_ISSUE(G8_B0, 1)
    G8_ISSUE(G8_B1, 1)
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    G8_ACC_FROM_BIAS(0)
    if (wr == 1) __builtin_amdgcn_s_barrier();   // wave row 1 runs one barrier behind wave row 0

    // fragment read offsets (bytes inside a slot): row r + 16 j keeps (r >> 1) & 7, so the rows of the j-th 16-row
    // tile are 2048 j bytes further; the second 32-wide k step is chunk ^ 4 = byte offset ^ 64
    // (ABLK: the A slot holds the blocked image itself -- block (wr, j) at (wr * 4 + j) * 2048, piece (c, lg, lq) of it at
    // c * 1024 + lane * 16: a fragment read is 1 KiB of contiguous LDS, conflict free without a swizzle)
    const int a_o0 = ABLK ? wr * 8192 + lane * 16 : swz_byte(wr * 64 + lq, lg), a_o1 = ABLK ? a_o0 + 1024 : (a_o0 ^ 64);
    const int b_o0 = (ABLK && G8_BBLK) ? wc * 4096 + lane * 16 : swz_byte(wc * 32 + lq, lg), b_o1 = (ABLK && G8_BBLK) ? b_o0 + 1024 : (b_o0 ^ 64);
    v4f a[4][2], b0[2][2], b1[2][2];
#define G8_READ_A(S_, D_)                                                                                     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                         \
        a[j][0] = *reinterpret_cast<const v4f*>(smem + ((D_) * 4 + ((S_) ? G8_A1 : G8_A0)) * G8_HT + j * 2048 + a_o0); \
        a[j][1] = *reinterpret_cast<const v4f*>(smem + ((D_) * 4 + ((S_) ? G8_A1 : G8_A0)) * G8_HT + j * 2048 + a_o1); \
    }
#define G8_READ_B(S_, D_, B_)                                                                                 \
    _Pragma("unroll") for (int n = 0; n < 2; ++n) {                                                         \
        B_[n][0] = *reinterpret_cast<const v4f*>(smem + ((D_) * 4 + ((S_) ? G8_B1 : G8_B0)) * G8_HT + n * 2048 + b_o0); \
        B_[n][1] = *reinterpret_cast<const v4f*>(smem + ((D_) * 4 + ((S_) ? G8_B1 : G8_B0)) * G8_HT + n * 2048 + b_o1); \
    }
// transposed product (MFMA rows <- W rows, columns <- tokens): a lane owns one token row and 4 consecutive columns
#define G8_MFMA(MH_, NH_, B_)                                                                                 \
    {                                                                                                         \
        __builtin_amdgcn_s_setprio(1);                                                                        \
        _Pragma("unroll") for (int c = 0; c < 2; ++c)                                                         \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                     \
                _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                 \
                    acc[4 * (MH_) + j][2 * (NH_) + n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(              \
                        __builtin_bit_cast(v8bf, B_[n][c]), __builtin_bit_cast(v8bf, a[j][c]),                \
                        acc[4 * (MH_) + j][2 * (NH_) + n], 0, 0, 0);                                          \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    }
#define G8_SYNC_A()                                   \
    __builtin_amdgcn_sched_barrier(0);                \
    __builtin_amdgcn_s_barrier();                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0);
#define G8_SYNC_B()                    \
    __builtin_amdgcn_sched_barrier(0); \
    __builtin_amdgcn_s_barrier();      \
    __builtin_amdgcn_sched_barrier(0);
    int ct_tile = 0, kt = 0;
    int flush_row0 = 0;   // EPI_RES: first row of this wave row's block in the tile whose statistics await G8_STATS_FLUSH
// row statistics of the current tile (in LDS since the previous tile's first K step): wave row 0 turns the 256 raw
// (sum, sum^2) pairs into (rs, mu rs) in place, once per tile, during the tile's second K step; the epilogues of all
// waves read them many barriers later.  (Inline-asm LDS access: see the header comment.)
#define G8_DECODE()                                                                                           \
    if ((AFF || RES) && kt == 1 && wr == 0) {                                                                 \
        const unsigned so_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&sbias[ct_tile & 1][2][(wave * 64 + lane) * 4]; \
        v4u32 raw_;                                                                                           \
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(raw_) : "v"(so_) : "memory");      \
        typedef float v2f_ __attribute__((ext_vector_type(2)));                                               \
        float rs_, mrs_;                                                                                      \
        row_stats_decode(raw_, side.inv_h, side.eps, rs_, mrs_);                                              \
        const v2f_ o_ = {rs_, mrs_};                                                                          \
        asm volatile("ds_write_b64 %0, %1" : : "v"(so_), "v"(o_) : "memory");                                 \
    }
// EPI_RES: statistics of the PREVIOUS tile (partials of the wave row's four waves in their transpose scratch since the
// end of that tile's epilogue; >= 20 block barriers ago for every wave) -> one fixed-order sum per row, then fixed-point
// integer atomics (the order in which tile columns arrive does not matter: bit-reproducible).  Wave wc handles slots
// 16 wc .. 16 wc + 15 (slot s = rows s and 64 + s of the 128-row block).
#define G8_STATS_FLUSH()                                                                                      \
    if constexpr (RES) {                                                                                      \
        if (lane < 16) {                                                                                      \
            const int sl_ = 16 * wc + lane;                                                                   \
            const unsigned fo_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(sepi[wr * 4] + sl_ * 16); \
            v4f q0_, q1_;                                                                                     \
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:%3\n\ts_waitcnt lgkmcnt(0)"        \
                         : "=&v"(q0_), "=&v"(q1_) : "v"(fo_), "n"(16 * EPI_ROW) : "memory");                  \
            v4f t_ = q0_ + q1_;                                                                               \
            asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)" \
                         : "=&v"(q0_), "=&v"(q1_) : "v"(fo_), "n"(32 * EPI_ROW), "n"(48 * EPI_ROW) : "memory"); \
            t_ += q0_ + q1_;                                                                                  \
            unsigned long long* so_ = reinterpret_cast<unsigned long long*>(side.stats_out) + (size_t)(flush_row0 + sl_) * 2; \
            atomicAdd(so_, (unsigned long long)__float2ll_rn(t_[0] * kStatScale1));                           \
            atomicAdd(so_ + 1, (unsigned long long)__float2ll_rn(t_[1] * kStatScale2));                       \
            atomicAdd(so_ + 128, (unsigned long long)__float2ll_rn(t_[2] * kStatScale1));                     \
            atomicAdd(so_ + 129, (unsigned long long)__float2ll_rn(t_[3] * kStatScale2));                     \
        }                                                                                                     \
    }
#define G8_KSTEP(D_)                                                                                          \
    {                                                                                                         \
        /* P1 */                                                                                              \
        G8_READ_B(0, D_, b0)                                                                                  \
        G8_READ_A(0, D_)                                                                                      \
        G8_ISSUE(G8_A1, (D_) ^ 1)                                                                             \
        G8_SYNC_A()                                                                                           \
        G8_MFMA(0, 0, b0)                                                                                     \
        G8_SYNC_B()                                                                                           \
        /* P2 */                                                                                              \
        G8_READ_B(1, D_, b1)                                                                                  \
        G8_ISSUE(G8_A0, D_)                                                                                   \
        if (kt == 0 && ct_tile + 1 < my_ntiles) G8_BIAS(ct_tile + 1)                                          \
        G8_SYNC_A()                                                                                           \
        G8_MFMA(0, 1, b1)                                                                                     \
        G8_SYNC_B()                                                                                           \
        /* P3 */                                                                                              \
        G8_DECODE()                                                                                           \
        G8_READ_A(1, D_)                                                                                      \
        G8_ISSUE(G8_B0, D_)                                                                                   \
        G8_SYNC_A()                                                                                           \
        G8_MFMA(1, 1, b1)                                                                                     \
        G8_SYNC_B()                                                                                           \
        /* P4 */                                                                                              \
        G8_ISSUE(G8_B1, D_)                                                                                   \
        if (g + 2 < total) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                                   \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                 \
        G8_SYNC_A()                                                                                           \
        G8_MFMA(1, 0, b0)                                                                                     \
        G8_SYNC_B()                                                                                           \
        /* (between K steps every fragment register is dead: the one place with room for the flush) */        \
        if (RES && kt == 2 && ct_tile > 0) G8_STATS_FLUSH()                                                   \
        ++g;                                                                                                  \
        ++kt;                                                                                                 \
    }

    for (int g = 0; g < total;) {
        G8_KSTEP(0)
        G8_KSTEP(1)
        if (kt == KT) {
            // ---- epilogue of output tile ct_tile (no block barrier inside: the stagger carries over)
            const int tile = G8_TILE(jx + ct_tile * per_x);
            const int col0 = (tile % ntn) * BN + wc * 64;
            const unsigned wbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(sepi[wave] + lq * EPI_ROW + 8 * lg);
            const unsigned rbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(sepi[wave] + (lane >> 3) * EPI_ROW + (lane & 7) * 16);
            bf16_t* cbase = Cout + (size_t)((tile / ntn) * BM + wr * 128 + (lane >> 3)) * N + col0 + (lane & 7) * 8;
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            float sc[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) sc[n] = (DO_QSCALE && col0 + 16 * n < qscale_cols) ? qscale : 1.0f;  // qscale_cols % 16 == 0
            const int par = ct_tile & 1;
            // AFF: d of this lane's 16 columns, rs of its 8 rows (inline-asm LDS reads: see header); the q scale is folded in
            v4f dj[4];
            float rs_m[8], mrs_m[8];
            if constexpr (AFF) {
                const unsigned so_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&sbias[par][0][wc * 64 + 4 * lg];
                asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\t"
                             "ds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(dj[0]), "=&v"(dj[1]), "=&v"(dj[2]), "=&v"(dj[3])
                             : "v"(so_) : "memory");
            }
            const unsigned rso_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&sbias[par][2][(wr * 128 + lq) * 4];
            if constexpr (AFF) {   // (rs, mu rs) of this lane's 8 rows, decoded by G8_DECODE (RES reads them row block by row block)
                const unsigned ro_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&sbias[par][2][(wr * 128 + lq) * 4];
                typedef float v2f __attribute__((ext_vector_type(2)));
                v2f st[8];
                asm volatile("ds_read_b64 %0, %8\n\tds_read_b64 %1, %8 offset:256\n\tds_read_b64 %2, %8 offset:512\n\t"
                             "ds_read_b64 %3, %8 offset:768\n\tds_read_b64 %4, %8 offset:1024\n\tds_read_b64 %5, %8 offset:1280\n\t"
                             "ds_read_b64 %6, %8 offset:1536\n\tds_read_b64 %7, %8 offset:1792\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(st[0]), "=&v"(st[1]), "=&v"(st[2]), "=&v"(st[3]), "=&v"(st[4]), "=&v"(st[5]), "=&v"(st[6]), "=&v"(st[7])
                             : "v"(ro_) : "memory");
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    rs_m[m] = st[m][0];
                    mrs_m[m] = st[m][1];
                }
            }
            if constexpr (AFF) {
#pragma unroll
                for (int n = 0; n < 4; ++n) dj[n] *= sc[n];
                // statistics the next EPI_RES GEMM adds into: zero this tile's rows (first tile column, wave column 0)
                if (tile % ntn == 0 && wc == 0) {
                    v4u* zp = reinterpret_cast<v4u*>(side.stats_out + (size_t)((tile / ntn) * BM + wr * 128) * 2);
                    zp[lane] = v4u{0u, 0u, 0u, 0u};
                    zp[lane + 64] = v4u{0u, 0u, 0u, 0u};
                }
            }
            // RES: gamma of this lane's 16 columns, (rs, mu rs) of its 8 rows, and the previous pre -- blocked layout
            // (preblk_elem): the 16-byte piece (j, lg, lq) of block (16-row block m of this wave row, this wave's 64 columns)
            // IS acc[m][2 j], acc[m][2 j + 1] of lane lq + 16 lg, so a wave instruction moves 1 KiB of contiguous bytes and
            // nothing goes through LDS (round 3: two transposes per 16-row block through the wave's scratch).  All 16 loads
            // are requested before the first store of the epilogue (a wave's loads return in order behind its stores).
            v4f gj[4];
            v4u pv[16];
            float keep[4] = {0.f, 0.f, 0.f, 0.f};   // row sums this lane reports: rows lq + 16 (lg + 4 j), (sum, sum^2)
            // OBLK: byte offset of this lane's piece (m = 0, j = 0) in the blocked output (and previous pre); stride of m
            const size_t blk_m = preblk_rowstride(N);
            const size_t blk_o = (size_t)(((tile / ntn) * BM + wr * 128) >> 4) * blk_m + (size_t)((tile % ntn) * 4 + wc) * 2048 + lane * 16;
            if constexpr (RES) {
                const unsigned go_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&sbias[par][1][wc * 64 + 4 * lg];
                asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\t"
                             "ds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                             : "=&v"(gj[0]), "=&v"(gj[1]), "=&v"(gj[2]), "=&v"(gj[3])
                             : "v"(go_) : "memory");
                const char* pb = reinterpret_cast<const char*>(side.pprev) + blk_o;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    pv[2 * m] = *reinterpret_cast<const v4u*>(pb + m * blk_m);
                    pv[2 * m + 1] = *reinterpret_cast<const v4u*>(pb + m * blk_m + 1024);
                }
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                uint2 pk[4];
                v4f s1v = {0.f, 0.f, 0.f, 0.f}, s2v = {0.f, 0.f, 0.f, 0.f};
                if constexpr (RES) {
                    if ((m & 3) == 0) {   // (rs, mu rs) of four row blocks at a time (all eight up front: 8 registers too many)
                        typedef float v2f __attribute__((ext_vector_type(2)));
                        v2f st[4];
                        asm volatile("ds_read_b64 %0, %4 offset:%5\n\tds_read_b64 %1, %4 offset:%6\n\tds_read_b64 %2, %4 offset:%7\n\t"
                                     "ds_read_b64 %3, %4 offset:%8\n\ts_waitcnt lgkmcnt(0)"
                                     : "=&v"(st[0]), "=&v"(st[1]), "=&v"(st[2]), "=&v"(st[3])
                                     : "v"(rso_), "n"(256 * m), "n"(256 * m + 256), "n"(256 * m + 512), "n"(256 * m + 768) : "memory");
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            rs_m[i] = st[i][0];
                            mrs_m[i] = st[i][1];
                        }
                    }
                }
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    v4f v = acc[m][n];
                    if constexpr (AFF) {
                        const float rsn = rs_m[m] * sc[n];
                        v = __builtin_elementwise_fma(v, v4f{rsn, rsn, rsn, rsn}, dj[n]);
                    }
                    if constexpr (RES) {
                        // acc holds branch + bias + beta; residual = gamma (p rs - mu rs) + beta
                        const unsigned pwx = pv[2 * m + (n >> 1)][2 * (n & 1)], pwy = pv[2 * m + (n >> 1)][2 * (n & 1) + 1];
                        v4f pf;
                        pf[0] = __uint_as_float(pwx << 16);
                        pf[1] = __uint_as_float(pwx & 0xFFFF0000u);
                        pf[2] = __uint_as_float(pwy << 16);
                        pf[3] = __uint_as_float(pwy & 0xFFFF0000u);
                        const float rs_ = rs_m[m & 3], mrs_ = mrs_m[m & 3];
                        const v4f u = __builtin_elementwise_fma(pf, v4f{rs_, rs_, rs_, rs_}, v4f{-mrs_, -mrs_, -mrs_, -mrs_});
                        v = __builtin_elementwise_fma(gj[n], u, v);
                        s1v += v;
                        s2v = __builtin_elementwise_fma(v, v, s2v);
                    }
                    if constexpr (DO_GELU) {
                        v = gelu_poly4(v);
                    } else if constexpr (DO_QSCALE && !AFF) {
                        v[0] *= sc[n]; v[1] *= sc[n]; v[2] *= sc[n]; v[3] *= sc[n];
                    }
                    pk[n].x = (unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
                    pk[n].y = (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
                }
                if constexpr (RES) {
                    // row sums over this wave's 64 columns: 4 values per lane, then the 4 lanes lg = 0..3 of the row
                    // (lane ^ 16, lane ^ 32: v_permlane16_swap / v_permlane32_swap on the VALU, no LDS crossbar)
                    float r1 = (s1v[0] + s1v[1]) + (s1v[2] + s1v[3]), r2 = (s2v[0] + s2v[1]) + (s2v[2] + s2v[3]);
                    {
                        const auto a1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(r1), __float_as_uint(r1), false, false);
                        const auto a2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(r2), __float_as_uint(r2), false, false);
                        r1 = __uint_as_float(a1[0]) + __uint_as_float(a1[1]);
                        r2 = __uint_as_float(a2[0]) + __uint_as_float(a2[1]);
                        const auto b1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(r1), __float_as_uint(r1), false, false);
                        const auto b2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(r2), __float_as_uint(r2), false, false);
                        r1 = __uint_as_float(b1[0]) + __uint_as_float(b1[1]);
                        r2 = __uint_as_float(b2[0]) + __uint_as_float(b2[1]);
                    }
                    if (lg == (m & 3)) {
                        keep[2 * (m >> 2)] = r1;
                        keep[2 * (m >> 2) + 1] = r2;
                    }
                }
                if constexpr (OBLK) {
                    // blocked layout: this lane's two 16-byte pieces of block m, straight from the registers
                    char* cb_ = reinterpret_cast<char*>(Cout) + blk_o + m * blk_m;
                    if constexpr (RES) {
                        // a pre tensor (151 MB at 256 x 384) is the A operand of the very next GEMM: plain stores leave it in the
                        // Infinity Cache for that reader (measured in one session: 18.64 -> 18.48 ms per forward; plain stores of
                        // the 450 / 600 MB qkv and FFN1 outputs, which cannot stay resident, cost 0.05 / 0.2 ms instead)
                        *reinterpret_cast<v4u*>(cb_) = v4u{pk[0].x, pk[0].y, pk[1].x, pk[1].y};
                        *reinterpret_cast<v4u*>(cb_ + 1024) = v4u{pk[2].x, pk[2].y, pk[3].x, pk[3].y};
                    } else {
                        __builtin_nontemporal_store(v4u{pk[0].x, pk[0].y, pk[1].x, pk[1].y}, reinterpret_cast<v4u*>(cb_));
                        __builtin_nontemporal_store(v4u{pk[2].x, pk[2].y, pk[3].x, pk[3].y}, reinterpret_cast<v4u*>(cb_ + 1024));
                    }
                } else {
                    v4u o0, o1;
                    asm volatile("ds_write_b64 %6, %2\n\tds_write_b64 %6, %3 offset:32\n\tds_write_b64 %6, %4 offset:64\n\t"
                                 "ds_write_b64 %6, %5 offset:96\n\ts_waitcnt lgkmcnt(0)\n\t"
                                 "ds_read_b128 %0, %7\n\tds_read_b128 %1, %7 offset:%8\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(o0), "=&v"(o1)
                                 : "v"(pk[0]), "v"(pk[1]), "v"(pk[2]), "v"(pk[3]), "v"(wbase), "v"(rbase), "n"(8 * EPI_ROW)
                                 : "memory");
                    __builtin_nontemporal_store(o0, reinterpret_cast<v4u*>(cbase + (size_t)(16 * m) * N));
                    __builtin_nontemporal_store(o1, reinterpret_cast<v4u*>(cbase + (size_t)(16 * m + 8) * N));
                }
            }
            if constexpr (RES) {
                // Row sums over this wave's 64 columns: lane (lq, lg) holds rows 16 lg + lq and 64 + 16 lg + lq of the wave
                // row's 128-row block, i.e. slot `lane` of a [64][4]-float array in the wave's transpose scratch.  The four
                // waves of a wave row are combined from there during the NEXT tile's third K step (G8_STATS_FLUSH): one
                // set of integer atomics per row and tile instead of four (round 2: every lane of every wave issued its
                // own 4 atomics, 0.26 ms per forward).
                const unsigned ko_ = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(sepi[wave] + lane * 16);
                asm volatile("ds_write2_b32 %0, %1, %2 offset1:1\n\tds_write2_b32 %0, %3, %4 offset0:2 offset1:3\n\ts_waitcnt lgkmcnt(0)"
                             : : "v"(ko_), "v"(keep[0]), "v"(keep[1]), "v"(keep[2]), "v"(keep[3]) : "memory");
                flush_row0 = __builtin_amdgcn_readfirstlane((tile / ntn) * BM + wr * 128);
            }
            // bias row of the NEXT tile (in LDS since P2 of this tile's first K step) -> accumulator start values
            G8_ACC_FROM_BIAS((ct_tile + 1) & 1)
            kt = 0;
            ++ct_tile;
        }
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();   // balance the stagger barrier of wave row 1
    if constexpr (RES) {   // statistics of the block's last tile
        __builtin_amdgcn_s_barrier();
        G8_STATS_FLUSH()
    }
#undef G8_STATS_FLUSH
#undef G8_KSTEP
#undef G8_SYNC_A
#undef G8_SYNC_B
#undef G8_MFMA
#undef G8_READ_A
#undef G8_READ_B
#undef G8_ACC_FROM_BIAS
#undef G8_BIAS
#undef G8_TILE
#undef G8_ISSUE
#undef G8_SET_SRC
}

// ---------------------------------------------------------------- skinny GEMM (M <= 64 tokens)
// The single-query path (generate_single_embedding, src/embeddings.py:179-190) is a
// weight-streaming problem: 85 MB of bf16 weights per forward, a few dozen tokens.  The big
// persistent kernel would run 12..48 latency-bound K-stages on a handful of CUs; here every
// block owns 32 output columns, its 4 waves split K four ways and stream their W slices
// straight into MFMA fragments (no LDS, deep load queue), then reduce through LDS.
// Same transposed product / epilogue semantics as k_gemm.
template <typename TIn, int EPI, int MT, int UNR = 12>
__global__ __launch_bounds__(256) void k_gemm_skinny(const TIn* __restrict__ A, const TIn* __restrict__ W,
                                                     const float* __restrict__ bias, void* __restrict__ Cout, int M,
                                                     int N, int K, int qscale_cols, float qscale) {
    constexpr bool BF = sizeof(TIn) == 2;
    constexpr int KS = 16 / (int)sizeof(TIn) * 2;  // K elements per 16-B fragment pair step: 16 (bf16) / 8 (f32)
    __shared__ float red[4][MT][16][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const int col0 = blockIdx.x * 32;
    const int kq = K / 4;  // this wave's K range
    const char* wp = reinterpret_cast<const char*>(W + (size_t)(col0 + fr) * K + wave * kq) + fh * 16;
    const char* ap[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int tok = 32 * m + fr;
        tok = tok < M ? tok : M - 1;
        ap[m] = reinterpret_cast<const char*>(A + (size_t)tok * K + wave * kq) + fh * 16;
    }
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    // groups of UNR fragment steps are loaded back to back (12 x 16 B of W and of each token
    // tile per lane in flight) before their MFMAs: the kernel lives on memory-level parallelism
    const int nsteps = kq / KS;  // multiple of UNR: 12 for K % 768 == 0, 6 for K = 384 (hidden 384; host check)
    for (int s0 = 0; s0 < nsteps; s0 += UNR) {
        v4f wf[UNR], af[MT][UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            wf[u] = *reinterpret_cast<const v4f*>(wp + (size_t)(s0 + u) * 32);
#pragma unroll
            for (int m = 0; m < MT; ++m) af[m][u] = *reinterpret_cast<const v4f*>(ap[m] + (size_t)(s0 + u) * 32);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if constexpr (BF) {
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, wf[u]),
                                                                    __builtin_bit_cast(v8bf, af[m][u]), acc[m], 0, 0, 0);
                } else {
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[u].x, af[m][u].x, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[u].y, af[m][u].y, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[u].z, af[m][u].z, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[u].w, af[m][u].w, acc[m], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][m][r][lane] = acc[m][r];
    __syncthreads();
    // 256 threads finish MT*16*64 elements: element (m, r, l): column = col0 + (r&3)+8(r>>2)+4(l>>5), token = 32m+(l&31)
    for (int e = tid; e < MT * 16 * 64; e += 256) {
        const int l = e & 63, r = (e >> 6) & 15, m = e >> 10;
        const int tok = 32 * m + (l & 31);
        if (tok >= M) continue;
        const int col = col0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        float v = ((red[0][m][r][l] + red[1][m][r][l]) + (red[2][m][r][l] + red[3][m][r][l])) + bias[col];
        const size_t o = (size_t)tok * N + col;
        if constexpr (EPI == EPI_RESID) {
            reinterpret_cast<float*>(Cout)[o] = v;
        } else {
            if constexpr (EPI == EPI_GELU) v = BF ? gelu_erf_fast(v) : gelu_erf(v);
            if constexpr (EPI == EPI_QKV) v *= col < qscale_cols ? qscale : 1.0f;
            if constexpr (BF) reinterpret_cast<bf16_t*>(Cout)[o] = f2bf(v);
            else reinterpret_cast<float*>(Cout)[o] = v;
        }
    }
}

// ---------------------------------------------------------------- attention (bf16, MFMA)
// Block = (sequence, 128-query block, head), 4 waves x 32 queries.  Swapped
// product S^T = K.Q^T keeps one query per lane (softmax in registers, one
// cross-half exchange); O^T = V^T.P^T takes P^T straight from the accumulator
// registers as the B operand (k order permuted: element j of lane half h is key
// 16s + 8(j>>2) + 4h + (j&3)); the matching V^T fragments come from a row-major V
// tile in LDS through ds_read_b64_tr_b16.  q is pre-scaled by log2(e)/8 in the QKV
// epilogue and bias_tab[h][rel + (maxL-1)] = log2(e) * W_rel[bucket(rel)][h] (rel = key - query):
// scores live in the log2 domain.
// (Measured alternatives: __launch_bounds__(256, 4) -- 120 instead of 150 registers, four blocks per CU -- took this
// latency-bound kernel from 3.1 to 2.46 ms per batch; a variant with one block per (sequence, head) and three
// 32-query groups per wave, staging K/V once, needs 239 registers and ran 4.1 ms: occupancy beats reuse here.)
// max over the two 32-lane halves (lane l <-> lane l ^ 32) on the VALU (v_permlane32_swap_b32: no LDS round trip).
// (Plain fmaxf on purpose: an inline-asm v_max3 directly behind the MFMAs would read their results without the wait
// states hipcc's hazard recognizer inserts for instructions it knows.)
__device__ __forceinline__ float halfmax(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// V tile in LDS: row-major 128-B rows whose 64-B halves are exchanged on rows with bit 1 set.  A ds_read_b64_tr_b16
// covers 4 consecutive key rows x 64 B per 32-lane group and banks are (a / 4) mod 64, i.e. rows r and r + 2 of a
// linear image collide (2-way conflict on every transposed read: SQ_LDS_BANK_CONFLICT 0.16 in round 2); with the
// exchange the four rows of a group land on four different 64-B quarters of the 256-B bank row.
__device__ __forceinline__ int vswz_byte(int row, int chunk) { return row * 128 + ((chunk ^ (((row >> 1) & 1) << 2)) << 4); }

// One pass over the keys of the block's (sequence, head) for this wave's 32 queries.  SAFE = false: the
// exponentials are taken WITHOUT a reference, p = exp2(score) (scores in the log2 domain), so a tile costs no
// running maximum, no vote, no branch and no subtraction: the bias values read from LDS land directly in the
// accumulators the QK^T MFMAs start from.  That is exact as long as the row sums stay inside the fp32 range; the
// caller checks sum in (2^-100, 2^100) for every query of the block and otherwise repeats the block with SAFE =
// true, the online softmax with a running maximum (reference 0 until a score exceeds it).  Attention logits of
// a trained encoder are a few tens at most (|score| < 69 = 100 ln 2 is the fast path's range), so the repeat is a
// guard, not a path that runs; tests force it with css_encoder_set_attention_range(e, 0).
// BLK: qkv is in the blocked layout of k_gemm8p's EPI_AFF_QKV epilogue (preblk_elem with H = 3 * hidden: head h of
// q / k / v = block column h / heads + h / 2 heads + h; 16-byte piece cl = 4 j + lg of a token = dims 32 j + 4 lg + {0..3}
// and 32 j + 16 + 4 lg + {0..3}).  K tile rows in LDS keep the pieces in piece order (the q fragments are the same pieces
// of the q block, so QK^T contracts matching dims); the V tile is kept as the block image itself with the 16-byte slots
// of piece row lg rotated by 4 lg (vblk_byte) and the transposed reads address ACTUAL dims, so the output is in
// natural dim order.  A staging wave instruction covers 4 pieces x 16 consecutive keys = 4 x 256 contiguous bytes.
__device__ __forceinline__ int vblk_byte(int key, int cl) {   // V tile (64 keys) in BLK mode: slot of piece cl of key
    return (key >> 4) * 2048 + (cl >> 2) * 1024 + (cl & 3) * 256 + (((key & 15) ^ ((cl & 3) << 2)) << 4);
}
// HD: head_dim 64, or 32 (BERT hidden 384; row-major qkv only): K / V tiles keep their 128-B LDS rows and use the first
// HD / 8 16-byte chunks of each (swizzles unchanged), QK^T takes HD / 16 K-steps of 32x32x16 and O^T = V^T.P^T is HD / 32
// output tiles of 32 dims.  BIAS = false (BERT): no position bias, the score accumulators start at 0 (SAFE: -mrun) and
// the block loads no bias table.
template <int HD, bool SAFE, bool BLK, bool BIAS>
__device__ __forceinline__ float attn_pass(const bf16_t* __restrict__ qkv, char* Ks, char* Vs, const float* bt, int tok0, int L,
                                           int head, int hidden, int maxL, int qic, const v4f (&qf)[4], f32x16 (&oacc)[2]) {
    static_assert(HD == 64 || (HD == 32 && !BLK), "head_dim 64, or 32 on row-major qkv");
    constexpr int CH = HD / 8;          // 16-byte chunks of a K / V row
    constexpr int SROWS = 256 / CH;     // key rows per staging pass (row-major qkv)
    constexpr int NPASS = 64 / SROWS;   // staging passes per 64-key tile
    constexpr int NKS = HD / 16, NMT = HD / 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int fr = lane & 31, fh = lane >> 5;
    const int ld = 3 * hidden;  // row stride of qkv in elements
    const int nkt = (L + 63) / 64;
    // staging, NPASS passes of SROWS keys x CH chunks.  Row-major qkv: CH lanes = the chunks of one key row.  BLK: 16 lanes
    // = one piece of 16 consecutive keys (even keys first: the K tile's swizzle then spreads 8 lanes over 8 bank groups)
    const int srow = BLK ? 2 * (tid & 7) + ((tid >> 3) & 1) + 16 * (tid >> 7) : tid / CH;
    const int schunk = BLK ? (tid >> 4) & 7 : tid % CH;
    const unsigned brs = (unsigned)(preblk_rowstride(ld) / 2);   // BLK: elements per 16-token block row (T * 3 hidden < 2^31)
    const unsigned poff = (unsigned)((schunk >> 2) * 512 + (schunk & 3) * 128);
    const bf16_t* kblk = qkv + (size_t)(head + hidden / 64) * 1024;
    const bf16_t* vblk = qkv + (size_t)(head + hidden / 32) * 1024;
    v4f rk[2], rv[2];
#define AT_GLOAD(KT_)                                                                               \
    _Pragma("unroll") for (int i = 0; i < NPASS; ++i) {                                             \
        int key = (KT_) * 64 + srow + SROWS * i;                                                    \
        key = key < L ? key : L - 1;                                                                \
        if constexpr (BLK) {   /* uniform base (k / v block column of this head) + a 32-bit element offset per lane */ \
            const unsigned t_ = (unsigned)(tok0 + key);                                             \
            const unsigned o_ = (t_ >> 4) * brs + (t_ & 15u) * 8u + poff;                           \
            rk[i] = *reinterpret_cast<const v4f*>(kblk + o_);                                       \
            rv[i] = *reinterpret_cast<const v4f*>(vblk + o_);                                       \
        } else {                                                                                    \
            const bf16_t* base = qkv + (size_t)(tok0 + key) * ld + head * HD + schunk * 8;          \
            rk[i] = *reinterpret_cast<const v4f*>(base + hidden);                                   \
            rv[i] = *reinterpret_cast<const v4f*>(base + 2 * hidden);                               \
        }                                                                                           \
    }
#define AT_SSTORE(BUF)                                                                              \
    _Pragma("unroll") for (int i = 0; i < NPASS; ++i) {                                             \
        *reinterpret_cast<v4f*>(Ks + (BUF) * 8192 + swz_byte(srow + SROWS * i, schunk)) = rk[i];    \
        *reinterpret_cast<v4f*>(Vs + (BUF) * 8192 + (BLK ? vblk_byte(srow + SROWS * i, schunk) : vswz_byte(srow + SROWS * i, schunk))) = rv[i]; \
    }
    // BLK: K / V tiles go global -> LDS by LDS-DMA (no staging registers, no ds_write): a tile is 4 key blocks x 2 KiB per
    // operand, wave w copies key block w in two 1-KiB pieces (4 pieces of 16 keys each).  The K tile is the block image
    // itself ([key block][piece cl][key]: a K fragment read is 16 lanes x 16 B contiguous, conflict free); the V tile is
    // the image with the keys of piece row lg rotated by 4 lg (vblk_byte): lane i of a piece fetches key (i & 15) ^ 4 lg.
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#define AT_DMA(KT_, BUF)                                                                            \
    _Pragma("unroll") for (int jp = 0; jp < 2; ++jp) {                                              \
        const int cl_ = 4 * jp + (lane >> 4);                                                       \
        const unsigned po_ = (unsigned)((cl_ >> 2) * 512 + (cl_ & 3) * 128);                        \
        int kk_ = (KT_) * 64 + 16 * wv + (lane & 15);                                               \
        int kv_ = (KT_) * 64 + 16 * wv + ((lane & 15) ^ ((cl_ & 3) << 2));                          \
        kk_ = kk_ < L ? kk_ : L - 1;                                                                \
        kv_ = kv_ < L ? kv_ : L - 1;                                                                \
        const unsigned tk_ = (unsigned)(tok0 + kk_), tv_ = (unsigned)(tok0 + kv_);                  \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kblk + ((tk_ >> 4) * brs + (tk_ & 15u) * 8u + po_)), \
            (__attribute__((address_space(3))) void*)(Ks + (BUF) * 8192 + wv * 2048 + jp * 1024), 16, 0, 0); \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vblk + ((tv_ >> 4) * brs + (tv_ & 15u) * 8u + po_)), \
            (__attribute__((address_space(3))) void*)(Vs + (BUF) * 8192 + wv * 2048 + jp * 1024), 16, 0, 0); \
    }
    if constexpr (BLK) {
        AT_DMA(0, 0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        AT_GLOAD(0)
        AT_SSTORE(0)
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[mt][r] = 0.f;
    float mrun = 0.f, lrun = 0.f;   // SAFE: mrun = reference of the exponentials = running maximum after the first tile

    // transposed V reads: lane 4q+p of a 16-lane group addresses key row +q, columns d0 + 4p .. 4p+3
    const int g16 = (lane >> 4) & 1, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int vflip = (q4 >> 1) & 1;   // = bit 1 of the key row (the other row terms are multiples of 4)
    const int vlane = (4 * fh + q4) * 128 + 32 * g16 + 8 * p4;   // + (16 st [+ 8]) * 128 + ((mt ^ vflip) * 64)
    // BLK: key row 16 (2 sub + st) + 4 fh + q4 (+ 8), dims 32 mt + 16 g16 + 4 p4 + {0..3} = half g16 of piece (j = mt, lg = p4):
    // block (2 sub + st) * 2048 + mt * 1024 + p4 * 256 + ((4 fh + q4 (+ 8)) ^ 4 p4) * 16 + 8 g16
    const int vlane_b = p4 * 256 + (((4 * fh + q4) ^ (4 * p4)) << 4) + 8 * g16;   // (+ 8 keys: slot ^ 8 = byte offset ^ 128)

    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt + 1 < nkt) {
            if constexpr (BLK) {
                AT_DMA(kt + 1, cur ^ 1)   // (buffer cur ^ 1 was last read in tile kt - 1, behind that tile's barrier)
            } else {
                AT_GLOAD(kt + 1)
            }
        }
        const char* Kb = Ks + cur * 8192;
        const char* Vb = Vs + cur * 8192;

#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int key0 = kt * 64 + sub * 32;
            if (key0 >= L) break;  // block-uniform
            // S^T[key][query] = K[key][:] . Q[query][:] + bias (- mrun): the accumulator STARTS at the bias from the LDS
            // table (SAFE: minus this query's running maximum), so the scores leave the MFMAs ready for the exponential.
            // Keys beyond the sequence start at -inf (last, partial tile only).  Scores are in the log2 domain: q was
            // pre-scaled by log2(e)/8 and bias_tab by log2(e), so the softmax uses v_exp_f32 (exp2) directly.
            f32x16 s;
            {
                if constexpr (BIAS) {
                    const float* bl = bt + (key0 + 4 * fh - qic + (maxL - 1));
#pragma unroll
                    for (int r = 0; r < 16; ++r) {   // (the table has 64 entries of padding)
                        if constexpr (SAFE) s[r] = bl[(r & 3) + 8 * (r >> 2)] - mrun;
                        else s[r] = bl[(r & 3) + 8 * (r >> 2)];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[r] = SAFE ? -mrun : 0.f;
                }
                if (key0 + 32 > L) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (key0 + 4 * fh + (r & 3) + 8 * (r >> 2) >= L) s[r] = -INFINITY;
                }
            }
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const v4f kf = *reinterpret_cast<const v4f*>(Kb + (BLK ? (2 * sub + (fr >> 4)) * 2048 + (2 * ks + fh) * 256 + (fr & 15) * 16
                                                                       : swz_byte(sub * 32 + fr, 2 * ks + fh)));
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8bf, kf), __builtin_bit_cast(v8bf, qf[ks]), s, 0, 0, 0);
            }
            if constexpr (SAFE) {
                float mloc = s[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) mloc = fmaxf(mloc, s[r]);
                mloc = halfmax(mloc);   // finite: key0 < L means at least one valid key
                // the reference moves when a score exceeds it (first tiles mostly) and always on the first tile, whose
                // reference was the arbitrary 0: shift the scores, rescale the running sums
                // (no tile summed yet: afterwards the query's sum is >= 1, the maximum's own term.  The test is on the sum of
                // BOTH lane halves: a half whose own terms all underflowed would otherwise take the first-tile branch a
                // second time, with a shift its partner does not make.)
                const bool first = lrun + __shfl_xor(lrun, 32) == 0.f;
                if (!__all(mloc <= 0.f && !first)) {
                    const float d = first ? mloc : fmaxf(mloc, 0.f);
                    // (first tile: the running sums are still 0 and are not rescaled -- with d = a hugely NEGATIVE lone
                    // maximum, e.g. a one-token sequence whose only logit is -1e4, exp2(-d) is inf and 0 * inf poisoned
                    // the row with NaN; later tiles have d >= 0, alpha <= 1)
                    const float alpha = first ? 0.f : __builtin_amdgcn_exp2f(-d);
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[r] -= d;
                    mrun += d;
                    lrun *= alpha;
#pragma unroll
                    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) oacc[mt][r] *= alpha;
                }
            }
            float lsum0 = 0.f, lsum1 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(s[r]), p1 = __builtin_amdgcn_exp2f(s[r + 1]);
                s[r] = p0;
                s[r + 1] = p1;
                lsum0 += p0;
                lsum1 += p1;
            }
            lrun += lsum0 + lsum1;
            // O^T[d][query] += V^T[d][key] . P^T[key][query]
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                v8bf pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (__bf16)s[8 * st + j];
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt) {
                    // lane (d = 32*mt + fr, half fh): keys {16st+4fh+0..3} and {16st+8+4fh+0..3}
                    // (BLK: the lane offset is made opaque per read pair: with plain loop-invariant addresses hipcc hoists
                    // the transposed reads of a whole tile, 248 bytes of scratch per lane and Q fragments reloaded in the loop)
                    int vo_ = vlane_b;
                    if constexpr (BLK) asm volatile("" : "+v"(vo_));
                    const char* vp = BLK ? Vb + vo_ + ((2 * sub + st) * 2048 + mt * 1024)
                                         : Vb + vlane + (sub * 32 + 16 * st) * 128 + ((mt ^ vflip) << 6);
                    const char* vp_hi = BLK ? Vb + (vo_ ^ 128) + ((2 * sub + st) * 2048 + mt * 1024) : vp + 8 * 128;
                    const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(vp));
                    const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(vp_hi));
                    // whole-vector shuffle + bitcast: per-element short -> __bf16 bitcasts of the
                    // tr-read result were miscompiled by hipcc 7.2 into a splat of element 0
                    const v8s both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                    const v8bf vf = __builtin_bit_cast(v8bf, both);
                    oacc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[mt], 0, 0, 0);
                }
            }
        }
        if constexpr (BLK) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the next tile have landed
        } else if (kt + 1 < nkt) {
            AT_SSTORE(cur ^ 1)
        }
        __syncthreads();
        cur ^= 1;
    }
#undef AT_GLOAD
#undef AT_SSTORE
#undef AT_DMA
    return lrun + __shfl_xor(lrun, 32);
}

// `range`: the fast pass is kept when every row sum lies in (1 / range, range); 0 forces the SAFE pass (tests).
// HD = 64 (MPNet, BERT-base) or 32 (BERT hidden 384, row-major qkv); BIAS = false: no position bias (BERT), dynamic LDS
// is then the K / V tiles alone (4 * 8192 bytes).
template <int HD, bool BLK, bool BIAS = true>
__global__ __launch_bounds__(256, 4) void k_attention_bf16(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                        const float* __restrict__ bias_tab, int maxL, int hidden,
                                                        bf16_t* __restrict__ ctx, int nqb, int heads, float range) {
    static_assert(HD == 64 || (HD == 32 && !BLK), "head_dim 64, or 32 on row-major qkv");
    constexpr int NKS = HD / 16, NMT = HD / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                 // [2][64 keys][128 B]  (swizzled)
    char* Vs = smem + 2 * 8192;      // [2][64 keys][128 B]  (row-major, halves exchanged: vswz_byte)
    float* bt = reinterpret_cast<float*>(smem + 4 * 8192);  // [2*maxL-1] + 64 (padding read by the last, partial tile); BIAS only

    // 1-D grid of B * nqb * heads blocks.  The nqb query blocks of one (sequence, head) read the same K / V rows:
    // they get consecutive slots of ONE XCD (blocks l, l + 8, l + 16, ... share an XCD under round-robin dispatch;
    // speed only), so K / V come from HBM once and from that XCD's L2 afterwards.
    const int nwork = gridDim.x;
    const int xcd = blockIdx.x & 7, ix = blockIdx.x >> 3;
    const int qx = nwork / 8, rx = nwork % 8;
    const int work = (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + ix;   // bijective (T1)
    const int qb = work % nqb, head = (work / nqb) % heads, b = work / (nqb * heads);
    const int tok0 = cu[b];
    const int L = cu[b + 1] - tok0;
    const int q0 = qb * 128;
    if (q0 >= L) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;

    // this lane's query (clamped for loads; invalid queries are not stored)
    const int qi = q0 + wave * 32 + fr;
    const int qic = qi < L ? qi : L - 1;
    // Q fragments as B operand: lane holds Q[query][16*ks + 8*fh + j]
    v4f qf[4] = {};
    {
        if constexpr (BLK) {   // piece cl = 2 ks + fh of this token's row in the q block of `head` (see attn_pass)
            const int t_ = tok0 + qic;
            const bf16_t* qp = qkv + (size_t)(t_ >> 4) * (preblk_rowstride(3 * hidden) / 2) + (size_t)head * 1024 + (t_ & 15) * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const v4f*>(qp + (ks >> 1) * 512 + (2 * (ks & 1) + fh) * 128);
        } else {
            const bf16_t* qp = qkv + (size_t)(tok0 + qic) * (3 * hidden) + head * HD;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const v4f*>(qp + 16 * ks + 8 * fh);
        }
    }
    if constexpr (BIAS) {
        const float* bsrc = bias_tab + (size_t)head * (2 * maxL - 1);
        for (int i = tid; i < 2 * maxL - 1 + 64; i += 256) bt[i] = i < 2 * maxL - 1 ? bsrc[i] : 0.f;
    }
    // The Q fragments are pinned HERE (a use the compiler has to wait for).  Without it hipcc's wait-count pass
    // cannot prove, at the QK^T MFMAs inside the loop, that the four Q loads have returned (vmcnt counts in order
    // and one path into the loop issues no tile loads), so it put vmcnt(3) .. vmcnt(0) in front of the four MFMAs of
    // every tile's first 32 keys -- every tile waited for the NEXT tile's global loads issued a few instructions
    // earlier, and the register prefetch hid nothing (round 2: 2.5 ms per batch).
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) asm volatile("" : "+v"(qf[ks]));

    f32x16 oacc[2];
    float ltot = 0.f;
    bool ok = false;
    if (range > 0.f) {
        ltot = attn_pass<HD, false, BLK, BIAS>(qkv, Ks, Vs, bt, tok0, L, head, hidden, maxL, qic, qf, oacc);
        ok = ltot < range && ltot * range > 1.0f;   // (NaN compares false)
    }
    if (!__syncthreads_and(ok)) ltot = attn_pass<HD, true, BLK, BIAS>(qkv, Ks, Vs, bt, tok0, L, head, hidden, maxL, qic, qf, oacc);
    const float inv = 1.0f / ltot;
    if constexpr (BLK) {
        // ctx in the blocked layout (preblk_elem, H = hidden; it is the O projection's A operand): lane (query fr, half fh)
        // holds dims 32 mt + 8 g + 4 fh + {0..3}; the 16-byte piece (j = mt, lg = 2 (g & 1) + fh) of its token pairs g and
        // g + 2.  Straight from the registers: 16 lanes (16 consecutive tokens) write 256 contiguous bytes.
        if (qi < L) {
            const int t_ = tok0 + qi;
            bf16_t* cp = ctx + (size_t)(t_ >> 4) * (preblk_rowstride(hidden) / 2) + (size_t)head * 1024 + (t_ & 15) * 8;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int gl = 0; gl < 2; ++gl) {
                    typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
                    v4u_ o;
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int g = gl + 2 * h2;
                        o[2 * h2] = (unsigned)f2bf(oacc[mt][4 * g + 0] * inv) | ((unsigned)f2bf(oacc[mt][4 * g + 1] * inv) << 16);
                        o[2 * h2 + 1] = (unsigned)f2bf(oacc[mt][4 * g + 2] * inv) | ((unsigned)f2bf(oacc[mt][4 * g + 3] * inv) << 16);
                    }
                    *reinterpret_cast<v4u_*>(cp + mt * 512 + (2 * gl + fh) * 128) = o;
                }
        }
        return;
    }
    // Output rows leave through a per-wave LDS transpose (the K / V tiles are dead: the pass ends with a block
    // barrier): a lane owns HALF a query row in 8-byte pieces, so direct stores scatter 8-B pieces over 64 rows per
    // instruction (store-issue bound: a quarter of a block's life in round 2); after the transpose 8 lanes write one
    // full 128-B line as 16-B stores.  Rows padded to 144 B (as k_gemm8p's epilogue).
    {
        constexpr int OROW = 144;
        constexpr int LPR = HD / 8, RPI = 64 / LPR;   // lanes per output row (16-B stores), rows per wave instruction
        char* ow = smem + wave * (32 * OROW);
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                ushort4 h;
                h.x = f2bf(oacc[mt][4 * g + 0] * inv);
                h.y = f2bf(oacc[mt][4 * g + 1] * inv);
                h.z = f2bf(oacc[mt][4 * g + 2] * inv);
                h.w = f2bf(oacc[mt][4 * g + 3] * inv);
                *reinterpret_cast<ushort4*>(ow + fr * OROW + (32 * mt + 8 * g + 4 * fh) * 2) = h;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // this wave's own LDS writes before its reads (no other wave touches the region)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int t = 0; t < 32 / RPI; ++t) {
            const int row = RPI * t + lane / LPR;
            const v4f o = *reinterpret_cast<const v4f*>(ow + row * OROW + (lane % LPR) * 16);
            const int q = q0 + wave * 32 + row;
            if (q < L) *reinterpret_cast<v4f*>(ctx + (size_t)(tok0 + q) * hidden + head * HD + (lane % LPR) * 8) = o;
        }
    }
}

// fp32 verification attention: one wave per (sequence, head, query); plain loops.  HD = head_dim (64 or 32: lane = output
// dim, lanes >= HD only take part in the score loop); bias_tab = nullptr: no position bias (BERT).
template <int HD>
__global__ __launch_bounds__(64) void k_attention_f32(const float* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                      const float* __restrict__ bias_tab, int maxL, int hidden,
                                                      float* __restrict__ ctx) {
    static_assert(HD == 64 || HD == 32, "head_dim 64 or 32");
    __shared__ float sc[512];
    const int b = blockIdx.x, head = blockIdx.z, qi = blockIdx.y;
    const int tok0 = cu[b];
    const int L = cu[b + 1] - tok0;
    if (qi >= L) return;
    const int lane = threadIdx.x;
    const int ld = 3 * hidden;
    const float* q = qkv + (size_t)(tok0 + qi) * ld + head * HD;  // already scaled by 1/sqrt(HD)
    const float* bt = bias_tab ? bias_tab + (size_t)head * (2 * maxL - 1) : nullptr;
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) {
        const float* kk = qkv + (size_t)(tok0 + j) * ld + hidden + head * HD;
        float s = 0.f;
        for (int d = 0; d < HD; ++d) s = fmaf(q[d], kk[d], s);
        if (bt) s += bt[j - qi + (maxL - 1)];
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int j = lane; j < L; j += 64) {
        const float p = expf(sc[j] - mx);
        sc[j] = p;
        sum += p;
    }
    sum = wave_allsum(sum);
    __syncthreads();
    if (lane >= HD) return;
    float o = 0.f;  // lane = output dim d
    for (int j = 0; j < L; ++j) o = fmaf(sc[j], qkv[(size_t)(tok0 + j) * ld + 2 * hidden + head * HD + lane], o);
    ctx[(size_t)(tok0 + qi) * hidden + head * HD + lane] = o / sum;
}

// ---------------------------------------------------------------- pooling
// Masked mean pooling + optional L2 normalise, deterministic two-stage reduction:
// k_pool_partial: grid (B, S) -- slice s of sequence b sums its share of the token rows into
//                 part[b][s][H] (coalesced row reads, fixed summation order);
// k_pool_final:   one block per sequence adds the S partial rows in order,
//                 e = sum / max(len, 1e-9), optional e / max(||e||, 1e-12).
template <int H>
__global__ __launch_bounds__(256) void k_pool_partial(const float* __restrict__ y, const int32_t* __restrict__ cu,
                                                      int S, float* __restrict__ part) {
    const int b = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const int t0 = cu[b], L = cu[b + 1] - t0;
    const int per = (L + S - 1) / S;
    const int lo = min(L, sl * per), hi = min(L, lo + per);
    constexpr int PER = (H + 255) / 256;
    float acc[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) acc[i] = 0.f;
    for (int t = lo; t < hi; ++t) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = tid + 256 * i;
            if (c < H) acc[i] += y[(size_t)(t0 + t) * H + c];
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = tid + 256 * i;
        if (c < H) part[((size_t)b * S + sl) * H + c] = acc[i];
    }
}

// LayerNorm-folded path: the rows are the last pre tensor (bf16) + its row statistics; the last LayerNorm is applied
// on the way:  sum_t LN(p_t)[c] = gamma[c] * sum_t (p_t[c] rs_t - mu_t rs_t) + n beta[c].
//
// pool_ln_rows: the blocked read of that sum, shared by k_pool_partial_ln and k_span_pool_ln.  For the GLOBAL token
// numbers [tb, te) it leaves red[q][c] = sum over the tokens t with t % 16 == q of (p_t[c] rs_t - mu_t rs_t), tokens in
// ascending order, and ends with a block barrier; pool_ln_col adds the 16 classes of a column in a fixed order.
// Blocked layout (preblk_elem): thread (lq = tid & 15, g = tid >> 4) reads the 16-byte pieces g, g + 16, ... of the
// tokens t with t % 16 == lq, so 16 consecutive lanes read 256 contiguous bytes.  256 threads.
template <int H>
__device__ __forceinline__ void pool_ln_rows(const bf16_t* __restrict__ pre, const long long* __restrict__ stats, float inv_h,
                                             float eps, int tb, int te, float (&red)[16][H + 8]) {
    static_assert(H % 128 == 0, "6 pieces per thread");
    constexpr int NP = H / 8, PT = NP / 16;   // pieces per token row / per thread
    const int tid = threadIdx.x;
    const int lq = tid & 15, g = tid >> 4;
    float acc[PT][8];
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
    for (int t = (tb & ~15) + lq; t < te; t += 16) {
        if (t < tb) continue;
        const v4u32 raw = *reinterpret_cast<const v4u32*>(stats + (size_t)t * 2);
        float rs, mrs;
        row_stats_decode(raw, inv_h, eps, rs, mrs);
        const char* row = reinterpret_cast<const char*>(pre) + (size_t)(t >> 4) * preblk_rowstride(H) + lq * 16;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int pi = g + 16 * i;
            const uint4 w = *reinterpret_cast<const uint4*>(row + (size_t)(pi >> 3) * 2048 + ((pi >> 2) & 1) * 1024 + (pi & 3) * 256);
            const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[i][2 * e] += fmaf(__uint_as_float(ww[e] << 16), rs, -mrs);
                acc[i][2 * e + 1] += fmaf(__uint_as_float(ww[e] & 0xFFFF0000u), rs, -mrs);
            }
        }
    }
    // piece pi holds columns 64 cb + 32 j + 4 lg + {0..3} and the same + 16
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const int pi = g + 16 * i;
        const int c0 = 64 * (pi >> 3) + 32 * ((pi >> 2) & 1) + 4 * (pi & 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[lq][c0 + e] = acc[i][e];
            red[lq][c0 + 16 + e] = acc[i][4 + e];
        }
    }
    __syncthreads();
}
template <int H>
__device__ __forceinline__ float pool_ln_col(const float (&red)[16][H + 8], int c) {
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a += red[i][c];
    return a;
}

template <int H>
__global__ __launch_bounds__(256) void k_pool_partial_ln(const bf16_t* __restrict__ pre, const long long* __restrict__ stats,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float inv_h, float eps, const int32_t* __restrict__ cu, int S,
                                                         float* __restrict__ part) {
    __shared__ float red[16][H + 8];
    const int b = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const int t0 = cu[b], L = cu[b + 1] - t0;
    const int per = (L + S - 1) / S;
    const int lo = min(L, sl * per), hi = min(L, lo + per);
    pool_ln_rows<H>(pre, stats, inv_h, eps, t0 + lo, t0 + hi, red);
    for (int c = tid; c < H; c += 256)
        part[((size_t)b * S + sl) * H + c] = fmaf(pool_ln_col<H>(red, c), gamma[c], (float)(hi - lo) * beta[c]);
}

template <int H>
__global__ __launch_bounds__(256) void k_pool_final(const float* __restrict__ part, const int32_t* __restrict__ cu,
                                                    int S, int normalize, float* __restrict__ out) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = cu[b + 1] - cu[b];
    constexpr int PER = (H + 255) / 256;
    float acc[PER];
    const float denom = fmaxf((float)L, 1e-9f);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = tid + 256 * i;
        float a = 0.f;
        if (c < H)
            for (int sl = 0; sl < S; ++sl) a += part[((size_t)b * S + sl) * H + c];
        acc[i] = a / denom;
        if (c < H) ss += acc[i] * acc[i];
    }
    ss = wave_allsum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-12f);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = tid + 256 * i;
        if (c < H) out[(size_t)b * H + c] = normalize ? acc[i] / nrm : acc[i];
    }
}

// CLS pooling (sentence-transformers Pooling with pooling_mode_cls_token): the row of token 0 of every sequence, then
// the optional e / max(||e||, 1e-12) of k_pool_final.  One block per sequence; thread tid owns columns tid + 256 i.
template <int H>
__device__ __forceinline__ void cls_pool_write(const float (&v)[(H + 255) / 256], int normalize, float* __restrict__ orow) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < (H + 255) / 256; ++i) ss += v[i] * v[i];   // (columns >= H hold 0)
    ss = wave_allsum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-12f);
#pragma unroll
    for (int i = 0; i < (H + 255) / 256; ++i) {
        const int c = tid + 256 * i;
        if (c < H) orow[c] = normalize ? v[i] / nrm : v[i];
    }
}

// fp32 token rows y [T][H] (the last LayerNorm's output)
template <int H>
__global__ __launch_bounds__(256) void k_pool_cls(const float* __restrict__ y, const int32_t* __restrict__ cu, int normalize,
                                                  float* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = y + (size_t)cu[b] * H;
    float v[(H + 255) / 256];
#pragma unroll
    for (int i = 0; i < (H + 255) / 256; ++i) {
        const int c = tid + 256 * i;
        v[i] = c < H ? row[c] : 0.f;
    }
    cls_pool_write<H>(v, normalize, out + (size_t)b * H);
}

// LayerNorm-folded path: the row is the last pre tensor (bf16, blocked layout) and the last LayerNorm is applied on the
// way with its row statistics, as k_pool_partial_ln does: LN(p)[c] = gamma[c] (p[c] rs - mu rs) + beta[c].
template <int H>
__global__ __launch_bounds__(256) void k_pool_cls_ln(const bf16_t* __restrict__ pre, const long long* __restrict__ stats,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float inv_h, float eps, const int32_t* __restrict__ cu, int normalize,
                                                     float* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = cu[b];
    const v4u32 raw = *reinterpret_cast<const v4u32*>(stats + (size_t)t * 2);
    float rs, mrs;
    row_stats_decode(raw, inv_h, eps, rs, mrs);
    float v[(H + 255) / 256];
#pragma unroll
    for (int i = 0; i < (H + 255) / 256; ++i) {
        const int c = tid + 256 * i;
        v[i] = c < H ? fmaf(gamma[c], fmaf(bf2f(pre[preblk_elem(t, c, H)]), rs, -mrs), beta[c]) : 0.f;
    }
    cls_pool_write<H>(v, normalize, out + (size_t)b * H);
}

// ---------------------------------------------------------------- cross-encoder head
// css_encoder_forward_pairs: logit[b] = dot(wc, tanh(Wp h_b + bp)) + bc over the CLS rows h [B][H] (fp32, from
// k_pool_cls / k_pool_cls_ln with normalize = 0).  fp32 in both compute modes, no atomics, every sum in a fixed order:
// the same batch gives the same bits.
//
// k_ce_head<H>: grid (tiles of kCeTile = 8 pairs, H / kCeSlab slabs of output rows), 256 threads.  The tile's CLS rows
// sit in LDS (8 x 768 x 4 B = 24 KiB), so Wp is read once per 8 pairs.  Wave w takes rows j = slab + w + 4 r of Wp,
// kCeRows at a time (their coalesced float4 loads are in flight together and one LDS read serves all of them), forms the
// 8 dot products per row against the LDS rows, reduces each across the lanes (wave_allsum), and accumulates
// wc[j] * tanhf(. + bp[j]) per pair in a register.  The four waves' partials are summed in a fixed order through LDS
// into part[tile][slab][pair].  The slabs exist because one block per tile walking all H rows measured 0.13 ms (H = 384)
// / 0.30 ms (H = 768) for 64 pairs -- 8 blocks on 256 CUs, each wave bound by its own 8 reductions and tanhf per row
// (DESIGN.md 3.3c).
// k_ce_head_sum: logit[b] = (part[..][0][..] + part[..][1][..] + ...) + bc, slabs in ascending order, bc last.
constexpr int kCeTile = 8;
constexpr int kCeRows = 4;              // output rows per wave and step
constexpr int kCeSlab = 3 * 4 * kCeRows;   // output rows per block: three steps of 4 waves x kCeRows (divides 384 and 768)
template <int H>
__global__ __launch_bounds__(256) void k_ce_head(const float* __restrict__ cls, const float* __restrict__ wp,
                                                 const float* __restrict__ bp, const float* __restrict__ wc, int B,
                                                 float* __restrict__ part_out) {
    static_assert(H % 128 == 0, "float4 columns of a row cover whole 32-lane halves");
    static_assert(H % kCeSlab == 0, "whole slabs of output rows");
    constexpr int NV = (H / 4 + 63) / 64;   // float4 per lane (k_embed_ln's column split)
    __shared__ float4 rows[kCeTile][H / 4];
    __shared__ float part[4][kCeTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * kCeTile, jb = blockIdx.y * kCeSlab;
    for (int i = tid; i < kCeTile * (H / 4); i += 256) {
        const int p = i / (H / 4), c = i - p * (H / 4);
        rows[p][c] = b0 + p < B ? reinterpret_cast<const float4*>(cls + (size_t)(b0 + p) * H)[c]
                                : make_float4(0.f, 0.f, 0.f, 0.f);   // (pairs beyond the batch: zero rows, never read back)
    }
    __syncthreads();
    float acc[kCeTile];
#pragma unroll
    for (int p = 0; p < kCeTile; ++p) acc[p] = 0.f;
    for (int j0 = jb + wave; j0 < jb + kCeSlab; j0 += 4 * kCeRows) {   // rows j0 + 4 r < jb + kCeSlab <= H
        float4 w[kCeRows][NV];
#pragma unroll
        for (int r = 0; r < kCeRows; ++r)
#pragma unroll
            for (int i = 0; i < NV; ++i)
                w[r][i] = ln_col_ok<H>(lane + 64 * i)
                              ? reinterpret_cast<const float4*>(wp + (size_t)(j0 + 4 * r) * H)[lane + 64 * i]
                              : make_float4(0.f, 0.f, 0.f, 0.f);
        float d[kCeRows][kCeTile];
#pragma unroll
        for (int r = 0; r < kCeRows; ++r)
#pragma unroll
            for (int p = 0; p < kCeTile; ++p) d[r][p] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            if (!ln_col_ok<H>(lane + 64 * i)) continue;
#pragma unroll
            for (int p = 0; p < kCeTile; ++p) {
                const float4 x = rows[p][lane + 64 * i];
#pragma unroll
                for (int r = 0; r < kCeRows; ++r)
                    d[r][p] = fmaf(w[r][i].w, x.w, fmaf(w[r][i].z, x.z, fmaf(w[r][i].y, x.y, fmaf(w[r][i].x, x.x, d[r][p]))));
            }
        }
#pragma unroll
        for (int r = 0; r < kCeRows; ++r) {   // rows in ascending order
            const float bj = bp[j0 + 4 * r], wj = wc[j0 + 4 * r];
#pragma unroll
            for (int p = 0; p < kCeTile; ++p) acc[p] = fmaf(wj, tanhf(wave_allsum(d[r][p]) + bj), acc[p]);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < kCeTile; ++p) part[wave][p] = acc[p];
    }
    __syncthreads();
    if (tid < kCeTile)
        part_out[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * kCeTile + tid] =
            ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

__global__ void k_ce_head_sum(const float* __restrict__ part, const float* __restrict__ bc, int B, int nslab,
                              float* __restrict__ logits) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* p = part + (size_t)(b / kCeTile) * nslab * kCeTile + (b % kCeTile);
    float s = p[0];
    for (int k = 1; k < nslab; ++k) s += p[(size_t)k * kCeTile];
    logits[b] = s + bc[0];
}

// ---------------------------------------------------------------- span pooling
// css_encoder_forward_spans: one pooled row per SPAN (sequence b, begin, end) of token rows -- always the masked MEAN of
// the final hidden states of tokens begin..end-1, also for a CLS-pooling model.  One block per span, 256 threads, thread
// tid owns columns tid + 256 i; every sum has a fixed order, so the same call gives the same bits.
//
// span_range: global token numbers [tb, te) of span s.  The host entry point validates its table before anything is
// enqueued; the clamps keep the reads of a table that the caller of the _dev entry point did not validate inside the batch.
__device__ __forceinline__ void span_range(const int32_t* __restrict__ spans, const int32_t* __restrict__ cu, int B, int s,
                                           int& tb, int& te) {
    const int b = min(max(spans[3 * s], 0), B - 1);
    const int t0 = cu[b], L = cu[b + 1] - t0;
    const int lo = min(max(spans[3 * s + 1], 0), L), hi = min(max(spans[3 * s + 2], lo), L);
    tb = t0 + lo;
    te = t0 + hi;
}

// sum[i] = sum over the span's n tokens of column tid + 256 i (0 for columns >= H).  e = sum / max(n, 1e-9), then
// e / max(||e||, 1e-12) when normalize (the norm as k_pool_final forms it: wave sum + four LDS partials); orow (may be
// NULL) gets the row, *score (q != NULL) the dot of q with the row as written.
template <int H>
__device__ __forceinline__ void span_write(const float (&sum)[(H + 255) / 256], int n, int normalize, const float* __restrict__ q,
                                           float* __restrict__ orow, float* __restrict__ score) {
    __shared__ float red[2][4];
    constexpr int PER = (H + 255) / 256;
    const int tid = threadIdx.x;
    const float denom = fmaxf((float)n, 1e-9f);
    float v[PER];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        v[i] = sum[i] / denom;
        ss += v[i] * v[i];
    }
    ss = wave_allsum(ss);
    if ((tid & 63) == 0) red[0][tid >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(red[0][0] + red[0][1] + red[0][2] + red[0][3]), 1e-12f);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = tid + 256 * i;
        if (normalize) v[i] = v[i] / nrm;
        if (c < H) {
            if (orow) orow[c] = v[i];
            if (q) d += q[c] * v[i];
        }
    }
    if (q == nullptr) return;   // (uniform over the block)
    d = wave_allsum(d);
    if ((tid & 63) == 0) red[1][tid >> 6] = d;
    __syncthreads();
    if (tid == 0) *score = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}

// Unfolded paths: y [T][H] fp32 token rows (x32).  A thread walks the span's rows in ascending order: a block reads
// whole rows, coalesced.
template <int H>
__global__ __launch_bounds__(256) void k_span_pool(const float* __restrict__ y, const int32_t* __restrict__ cu, int B,
                                                   const int32_t* __restrict__ spans, int normalize,
                                                   const float* __restrict__ q, float* __restrict__ out,
                                                   float* __restrict__ scores) {
    const int s = blockIdx.x, tid = threadIdx.x;
    int tb, te;
    span_range(spans, cu, B, s, tb, te);
    constexpr int PER = (H + 255) / 256;
    float acc[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) acc[i] = 0.f;
    // rows in ascending order, the loads of RB rows in flight at once (a row at a time costs one memory round trip per
    // row); rows past the end add +0, which leaves every bit of the sum alone
    constexpr int RB = 8;
    for (int t = tb; t < te; t += RB) {
        float r[RB][PER];
#pragma unroll
        for (int j = 0; j < RB; ++j)
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int c = tid + 256 * i;
                r[j][i] = (c < H && t + j < te) ? y[(size_t)(t + j) * H + c] : 0.f;
            }
#pragma unroll
        for (int j = 0; j < RB; ++j)
#pragma unroll
            for (int i = 0; i < PER; ++i) acc[i] += r[j][i];
    }
    span_write<H>(acc, te - tb, normalize, q, out ? out + (size_t)s * H : nullptr, scores ? scores + s : nullptr);
}

// LayerNorm-folded path: the rows are the last pre tensor (bf16, blocked layout) + its row statistics, read through
// pool_ln_rows (token classes t % 16 over GLOBAL token numbers) with the last LayerNorm applied on the way, exactly as
// k_pool_partial_ln does it: sum = gamma[c] * sum_t (p_t[c] rs_t - mu_t rs_t) + n beta[c].
template <int H>
__global__ __launch_bounds__(256) void k_span_pool_ln(const bf16_t* __restrict__ pre, const long long* __restrict__ stats,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float inv_h, float eps, const int32_t* __restrict__ cu, int B,
                                                      const int32_t* __restrict__ spans, int normalize,
                                                      const float* __restrict__ q, float* __restrict__ out,
                                                      float* __restrict__ scores) {
    static_assert(H % 256 == 0, "thread tid owns columns tid + 256 i");
    __shared__ float red[16][H + 8];
    const int s = blockIdx.x, tid = threadIdx.x;
    int tb, te;
    span_range(spans, cu, B, s, tb, te);
    pool_ln_rows<H>(pre, stats, inv_h, eps, tb, te, red);
    float acc[H / 256];
#pragma unroll
    for (int i = 0; i < H / 256; ++i) {
        const int c = tid + 256 * i;
        acc[i] = fmaf(pool_ln_col<H>(red, c), gamma[c], (float)(te - tb) * beta[c]);
    }
    span_write<H>(acc, te - tb, normalize, q, out ? out + (size_t)s * H : nullptr, scores ? scores + s : nullptr);
}

// ---------------------------------------------------------------- token vectors (late interaction)
// css_encoder_forward_tokens: one bf16 row per TOKEN, tok[t] = W h_t (W [P][H] fp32, the ColBERT `linear.weight`) or
// h_t itself (W == NULL, P = H), then v / max(||v||, 1e-12) when normalize, rounded to bf16 once.  One block of 256
// threads per 16 consecutive GLOBAL tokens -- one block row of the blocked layout, so the folded path reads it through
// pool_ln_rows, where every class t % 16 then holds exactly one token.  No atomics, every sum in a fixed order.
//
// tok_write, the epilogue both kernels share: rows[q][c] = the fp32 LayerNorm output of token t0 + q (barrier done).
// Projection on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains; DESIGN.md 3.3d has the measurement): tokens are the rows
// of A, 16 rows of W the columns of B, wave w takes the column tiles w, w + 4.  A lane reads float4 at k0 + 4 (lane >> 4)
// from its token row (LDS) and its W row (global, L2 resident) and feeds the four elements to four MFMAs: the k
// assignment only has to agree between A and B.  Two accumulators alternate (the dependent latency of this MFMA is
// longer than its issue interval) and are added at the end.
constexpr int kTokMaxP = 128;   // widest projection
template <int H>
__device__ __forceinline__ void tok_write(const float (&rows)[16][H + 8], int t0, int T, const float* __restrict__ W, int P,
                                          int normalize, bf16_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float proj[16][kTokMaxP + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (W != nullptr) {   // (uniform over the grid)
        const int r = lane & 15, g = lane >> 4;
        for (int n = wave; n < P / 16; n += 4) {
            v4f acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const float* wrow = W + (size_t)(n * 16 + r) * H + 4 * g;
#pragma unroll 4
            for (int k0 = 0; k0 < H; k0 += 16) {
                const float4 a = *reinterpret_cast<const float4*>(&rows[r][k0 + 4 * g]);
                const float4 w = *reinterpret_cast<const float4*>(wrow + k0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc1, 0, 0, 0);
            }
            // C/D: column (output) lane & 15, row (token) 4 (lane >> 4) + i
#pragma unroll
            for (int i = 0; i < 4; ++i) proj[4 * g + i][n * 16 + r] = acc0[i] + acc1[i];
        }
        __syncthreads();
    }
    // thread (token tid >> 4, sub = tid & 15) owns the column pairs 2 sub + 32 i of its token
    const int tok = tid >> 4, sub = tid & 15;
    const float* src = W != nullptr ? &proj[tok][0] : &rows[tok][0];
    float ss = 0.f;
    for (int c = 2 * sub; c < P; c += 32) ss += src[c] * src[c] + src[c + 1] * src[c + 1];
    ss = row16_allsum(ss);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    if (t0 + tok >= T) return;
    unsigned* orow = reinterpret_cast<unsigned*>(out + (size_t)(t0 + tok) * P);
    for (int c = 2 * sub; c < P; c += 32) {
        const float a = normalize ? src[c] / nrm : src[c], b = normalize ? src[c + 1] / nrm : src[c + 1];
        orow[c >> 1] = (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16);
    }
}

// Unfolded paths: y [T][H] fp32 token rows (x32).
template <int H>
__global__ __launch_bounds__(256) void k_tok_vec(const float* __restrict__ y, int T, const float* __restrict__ W, int P,
                                                 int normalize, bf16_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float rows[16][H + 8];
    const int t0 = blockIdx.x * 16, tid = threadIdx.x;
    for (int i = tid; i < 16 * (H / 4); i += 256) {
        const int r = i / (H / 4), c = i - r * (H / 4);
        // (tokens beyond the batch: zero rows, never written back)
        *reinterpret_cast<float4*>(&rows[r][4 * c]) =
            t0 + r < T ? reinterpret_cast<const float4*>(y + (size_t)(t0 + r) * H)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    tok_write<H>(rows, t0, T, W, P, normalize, out);
}

// LayerNorm-folded path: the last pre tensor (bf16, blocked layout) + its row statistics through pool_ln_rows over the
// tokens [t0, t0 + 16): class q holds token t0 + q alone (0 + x is x), and the last LayerNorm is finished as
// k_pool_cls_ln does it: gamma[c] (p[c] rs - mu rs) + beta[c].
template <int H>
__global__ __launch_bounds__(256) void k_tok_vec_ln(const bf16_t* __restrict__ pre, const long long* __restrict__ stats,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float inv_h, float eps, int T, const float* __restrict__ W, int P,
                                                    int normalize, bf16_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float rows[16][H + 8];
    const int t0 = blockIdx.x * 16, tid = threadIdx.x;
    pool_ln_rows<H>(pre, stats, inv_h, eps, t0, min(t0 + 16, T), rows);
    for (int i = tid; i < 16 * H; i += 256) {
        const int r = i / H, c = i - r * H;
        rows[r][c] = fmaf(gamma[c], rows[r][c], beta[c]);
    }
    __syncthreads();
    tok_write<H>(rows, t0, T, W, P, normalize, out);
}

// ---------------------------------------------------------------- MaxSim (late interaction)
// css_encoder_maxsim: score(pair) = sum over the query's tokens s (ascending, fp32) of the maximum over the doc's kept
// tokens t of dot(q_s, d_t); bf16 rows of P elements, fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
// Grid (pairs, nsplit), blocks of four waves: block y of a pair takes the doc's tiles of 16 tokens 4 y + w,
// 4 (y + nsplit) + w, ... (w = its wave).  The host picks nsplit so that few pairs still fill the device (launch_maxsim).
// The query's rows (<= 64) sit in LDS, rows padded by 16 bytes so that the 16 lanes of a ds_read_b128 group fall into
// different banks; the doc's rows stream through from global memory.  A = query tokens (rows), B = doc tokens (columns): lane l reads 16 bytes at k = 32 s + 8 (l >> 4)
// of query row 16 mt + (l & 15) and of doc row 16 tile + (l & 15), and holds C/D of doc column l & 15 for the query rows
// 16 mt + 4 (l >> 4) + i.  Doc rows past the end are read from the doc's last row and, like the rows with keep == 0,
// enter the running maximum as -inf.  The maximum is reduced over the 16 lanes of a row group with DPP (row16_allmax),
// over the waves through LDS.  nsplit == 1: thread 0 adds the maxima in ascending s.  nsplit > 1: the block leaves its
// 64 maxima in part[pair][y][64] and k_maxsim_sum takes the maximum over y and adds in ascending s.  A maximum is
// order-free and the sum has one order, so the bits do not depend on the split.  Indices are clamped into range (the _dev entry point cannot check
// them); a doc without a kept token, or an empty query or doc, scores 0.
constexpr int kMaxsimQ = 64;   // query tokens at most
template <int P>
constexpr int maxsim_lds_bytes() { return kMaxsimQ * (P * 2 + 16) + 4 * kMaxsimQ * 4; }
__device__ __forceinline__ float row16_allmax(float v) {   // the DPP steps of row16_allsum
    v = fmaxf(v, dpp_f32<0xB1>(v));
    v = fmaxf(v, dpp_f32<0x4E>(v));
    v = fmaxf(v, dpp_f32<0x141>(v));
    v = fmaxf(v, dpp_f32<0x140>(v));
    return v;
}
template <int P>
__global__ __launch_bounds__(256) void k_maxsim(const bf16_t* __restrict__ q_tok, const int32_t* __restrict__ cu_q, int nq,
                                                const bf16_t* __restrict__ d_tok, const int32_t* __restrict__ cu_d, int nd,
                                                const uint8_t* __restrict__ keep, const int32_t* __restrict__ pairs,
                                                float* __restrict__ scores, float* __restrict__ part) {
    static_assert(P % 32 == 0, "whole K steps of the MFMA");
    constexpr int QS = P * 2 + 16;   // bytes per query row in LDS
    extern __shared__ __attribute__((aligned(16))) char maxsim_smem[];
    char* qs = maxsim_smem;
    float* wmax = reinterpret_cast<float*>(maxsim_smem + kMaxsimQ * QS);   // [4][kMaxsimQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.x, y = blockIdx.y, nsplit = gridDim.y;
    const int qi = min(max(pairs[2 * pair], 0), nq - 1), dj = min(max(pairs[2 * pair + 1], 0), nd - 1);
    const int q0 = cu_q[qi], mq = min(cu_q[qi + 1] - q0, kMaxsimQ);
    const int d0 = cu_d[dj], md = cu_d[dj + 1] - d0;
    if (mq <= 0 || md <= 0) {   // (uniform over the block; nsplit > 1: -inf maxima, which k_maxsim_sum scores 0)
        if (nsplit == 1 && tid == 0) scores[pair] = 0.f;
        if (nsplit > 1 && tid < kMaxsimQ) part[((size_t)pair * nsplit + y) * kMaxsimQ + tid] = -__builtin_inff();
        return;
    }
    const int MT = (mq + 15) >> 4;
    for (int i = tid; i < MT * 16 * (P / 8); i += 256) {
        const int r = i / (P / 8), c = i - r * (P / 8);
        // (rows beyond the query inside its last tile: zeros; their results are never read)
        *reinterpret_cast<uint4*>(qs + r * QS + 16 * c) =
            r < mq ? *reinterpret_cast<const uint4*>(q_tok + (size_t)(q0 + r) * P + 8 * c) : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const float ninf = -__builtin_inff();
    const int lr = lane & 15, g = lane >> 4;
    v4f run[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) run[mt] = v4f{ninf, ninf, ninf, ninf};
    // This wave's tiles are first, first + stride, ...; a tile's K steps go in chunks of CH.  The doc fragments of chunk
    // it + 1 (of the same tile or the next) are loaded before the MFMAs of chunk it, so a wave never waits for one
    // tile's loads with nothing else in flight.
    constexpr int KS = P / 32, CH = KS < 4 ? KS : 4, NCH = KS / CH;
    static_assert(KS % CH == 0, "whole chunks");
    const int ntiles = (md + 15) >> 4;
    const int first = 4 * y + wave, stride = 4 * nsplit;
    const int total = ntiles > first ? (ntiles - first + stride - 1) / stride * NCH : 0;
    const char* qrow = qs + lr * QS + 16 * g;
    auto load_chunk = [&](int it, v8s(&b)[CH]) {
        const int tile = first + stride * (it / NCH), c = it % NCH;
        const bf16_t* drow = d_tok + ((size_t)d0 + min(tile * 16 + lr, md - 1)) * P + 8 * g + 32 * CH * c;
#pragma unroll
        for (int j = 0; j < CH; ++j) b[j] = *reinterpret_cast<const v8s*>(drow + 32 * j);
    };
    v8s cur[CH], nxt[CH];
    if (total > 0) load_chunk(0, cur);
    v4f acc[4];
    for (int it = 0; it < total; ++it) {
        if (it + 1 < total) load_chunk(it + 1, nxt);
        const int tile = first + stride * (it / NCH), c = it % NCH;
        if (c == 0) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = v4f{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                if (mt < MT) {   // (uniform over the block)
                    const v8s a = *reinterpret_cast<const v8s*>(qrow + mt * 16 * QS + 64 * (CH * c + j));
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, cur[j]),
                                                                      acc[mt], 0, 0, 0);
                }
            }
        }
        if (c == NCH - 1) {
            const int tok = tile * 16 + lr;
            const bool ok = tok < md && (keep == nullptr || keep[(size_t)d0 + tok] != 0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) run[mt][i] = fmaxf(run[mt][i], ok ? acc[mt][i] : ninf);
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) cur[j] = nxt[j];
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float m = row16_allmax(run[mt][i]);
            if (lr == 0) wmax[wave * kMaxsimQ + mt * 16 + 4 * g + i] = m;
        }
    __syncthreads();
    if (tid < kMaxsimQ)
        wmax[tid] = fmaxf(fmaxf(wmax[tid], wmax[kMaxsimQ + tid]), fmaxf(wmax[2 * kMaxsimQ + tid], wmax[3 * kMaxsimQ + tid]));
    if (nsplit > 1) {   // (uniform over the grid)
        if (tid < kMaxsimQ) part[((size_t)pair * nsplit + y) * kMaxsimQ + tid] = wmax[tid];
        return;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int i = 0; i < mq; ++i) s += wmax[i];
        scores[pair] = wmax[0] == ninf ? 0.f : s;
    }
}

// The second step of a split MaxSim: one block of 64 threads per pair; thread s takes the maximum of query token s over
// the nsplit partial rows, thread 0 adds the maxima in ascending s as k_maxsim does.
__global__ __launch_bounds__(64) void k_maxsim_sum(const float* __restrict__ part, int nsplit, const int32_t* __restrict__ cu_q,
                                                   int nq, const int32_t* __restrict__ pairs, float* __restrict__ scores) {
    __shared__ float mx[kMaxsimQ];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int qi = min(max(pairs[2 * pair], 0), nq - 1);
    const int mq = min(cu_q[qi + 1] - cu_q[qi], kMaxsimQ);
    float m = -__builtin_inff();
    for (int y = 0; y < nsplit; ++y) m = fmaxf(m, part[((size_t)pair * nsplit + y) * kMaxsimQ + tid]);
    mx[tid] = m;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int i = 0; i < mq; ++i) s += mx[i];
        scores[pair] = (mq <= 0 || mx[0] == -__builtin_inff()) ? 0.f : s;
    }
}

// ---------------------------------------------------------------- learned sparse encoding (masked-LM head)
// css_encoder_forward_sparse: u_t = gelu(Wd h_t + bd) comes from the encoder's GEMMs; k_mlm_ln is the head's LayerNorm,
// k_layernorm without a residual: g_t = LayerNorm(u_t) as fp32 rows (out32) and / or rounded to bf16 once (out16).
template <int H, typename TIn>
__global__ __launch_bounds__(256) void k_mlm_ln(const TIn* __restrict__ in, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float eps, float* __restrict__ out32,
                                                bf16_t* __restrict__ out16, int T) {
    static_assert(H % 128 == 0, "float4 columns of a row cover whole 32-lane halves");
    constexpr int NV = (H / 4 + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const TIn* xrow = in + (size_t)t * H;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        v[i] = ln_load4<TIn>(xrow, lane + 64 * i);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_allsum(s) * (1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
        q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = rsqrtf(wave_allsum(q) * (1.0f / H) + eps);
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!ln_col_ok<H>(lane + 64 * i)) continue;
        const float4 g = g4[lane + 64 * i], b = b4[lane + 64 * i];
        float4 o;
        o.x = (v[i].x - mean) * rstd * g.x + b.x;
        o.y = (v[i].y - mean) * rstd * g.y + b.y;
        o.z = (v[i].z - mean) * rstd * g.z + b.z;
        o.w = (v[i].w - mean) * rstd * g.w + b.w;
        if (out32) reinterpret_cast<float4*>(out32 + (size_t)t * H)[lane + 64 * i] = o;
        if (out16) {
            ushort4 h;
            h.x = f2bf(o.x); h.y = f2bf(o.y); h.z = f2bf(o.z); h.w = f2bf(o.w);
            reinterpret_cast<ushort4*>(out16 + (size_t)t * H)[lane + 64 * i] = h;
        }
    }
}

// Vocabulary maximum: zmax[b][v] = max over the tokens t of sequence b of relu(dot(E_v, g_t) + c_v), the [T, V] logits
// never leaving the registers.  zmax holds the BIT PATTERNS of non-negative floats (zero-filled by the launcher): they
// order like unsigned integers, so the maximum across waves and blocks is one unsigned atomic maximum, which is
// order-free: the same call gives the same bits.  Only logits > 0 are sent.
//
// Grid (ceil(V / 128), ceil(T / 128)), four waves, wave w the 64 tokens x 64 terms at (64 (w >> 1), 64 (w & 1)) of the
// block's tile: A = token rows, B = rows of E, both K-contiguous and read from global memory (L1 / L2) one K step ahead
// of the MFMAs; a lane reads VmOp::KL elements at k0 + KL (lane >> 4) of token row 16 mt + (lane & 15) and of term row
// 16 nt + (lane & 15) and holds C/D of term lane & 15 for the tokens 16 mt + 4 (lane >> 4) + i.  Rows past T and terms
// past V are read from the last row (never out of bounds) and never written.
// Epilogue.  The wave's 64 tokens lie in one sequence (the usual case): the maximum over the 16 registers of a term,
// then over the four lane groups (two shuffles), c_v added after it (x + c is monotone in x, so the maximum commutes),
// and ONE atomic wave instruction over 64 consecutive terms.  A sequence boundary inside the 64 tokens: every lane
// finds the sequence of each of its tokens by bisection of cu_seqlens and sends its positive logits one by one --
// slow for many very short sequences, and exact.  Sequence numbers are clamped into [0, B), so a bad cu_seqlens on
// the _dev path cannot write outside zmax.
template <typename TIn>
struct VmOp;
template <>
struct VmOp<bf16_t> {   // v_mfma_f32_16x16x32_bf16
    typedef v8s frag;
    static constexpr int KS = 32, KL = 8;
    static __device__ __forceinline__ void mma(const frag& a, const frag& b, v4f& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), acc, 0, 0, 0);
    }
};
template <>
struct VmOp<float> {   // four v_mfma_f32_16x16x4_f32 per float4 (the k assignment only has to agree between A and B)
    typedef float4 frag;
    static constexpr int KS = 16, KL = 4;
    static __device__ __forceinline__ void mma(const frag& a, const frag& b, v4f& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
};

// the sequence b with cu[b] <= row < cu[b + 1] (lengths >= 1: cu is strictly increasing), clamped into [0, B)
__device__ __forceinline__ int vm_seq_of(const int32_t* __restrict__ cu, int B, int row) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cu[mid] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename TIn>
__global__ __launch_bounds__(256) void k_vocab_max(const TIn* __restrict__ g, const int32_t* __restrict__ cu, int B, int T,
                                                   const TIn* __restrict__ E, const float* __restrict__ cvec, int V, int H,
                                                   unsigned* __restrict__ zmax) {
    typedef typename VmOp<TIn>::frag frag;
    constexpr int KS = VmOp<TIn>::KS, KL = VmOp<TIn>::KL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int r0 = blockIdx.y * 128 + 64 * (wave >> 1), c0 = blockIdx.x * 128 + 64 * (wave & 1);
    if (r0 >= T || c0 >= V) return;   // (uniform over the wave; no barrier follows)
    const TIn* arow[4];
    const TIn* brow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        arow[j] = g + (size_t)min(r0 + 16 * j + lr, T - 1) * H + KL * lg;
        brow[j] = E + (size_t)min(c0 + 16 * j + lr, V - 1) * H + KL * lg;
    }
    v4f acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = v4f{0.f, 0.f, 0.f, 0.f};
    frag a[4], b[4], an[4], bn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = *reinterpret_cast<const frag*>(arow[j]);
        b[j] = *reinterpret_cast<const frag*>(brow[j]);
    }
    for (int k0 = 0; k0 < H; k0 += KS) {   // H is a multiple of KS (384, 768)
        const int kn = k0 + KS < H ? k0 + KS : k0;   // (the last step reloads its own fragments: no read past a row)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            an[j] = *reinterpret_cast<const frag*>(arow[j] + kn);
            bn[j] = *reinterpret_cast<const frag*>(brow[j] + kn);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) VmOp<TIn>::mma(a[mt], b[nt], acc[mt][nt]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = an[j];
            b[j] = bn[j];
        }
    }
    const int rlast = min(r0 + 64, T) - 1;
    const int b_lo = vm_seq_of(cu, B, r0), b_hi = vm_seq_of(cu, B, rlast);
    if (b_lo == b_hi) {
        // (rows past T repeat row T - 1, a token of this same sequence: they need no mask)
        float red[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            float m = acc[0][nt][0];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) m = fmaxf(m, acc[mt][nt][i]);
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            red[nt] = m;
        }
        // lane l takes term c0 + l: the column group lane >> 4 of the value that lane (l & 15) of every group holds
        const float m = lg == 0 ? red[0] : lg == 1 ? red[1] : lg == 2 ? red[2] : red[3];
        const int col = c0 + lane;
        if (col < V) {
            const float z = m + cvec[col];
            if (z > 0.f) atomicMax(zmax + (size_t)b_lo * V + col, __float_as_uint(z));
        }
        return;
    }
    int seq[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 16 * mt + 4 * lg + i;
            seq[mt][i] = row < T ? vm_seq_of(cu, B, row) : -1;
        }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int col = c0 + 16 * nt + lr;
        if (col >= V) continue;
        const float cv = cvec[col];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float z = acc[mt][nt][i] + cv;
                if (seq[mt][i] >= 0 && z > 0.f) atomicMax(zmax + (size_t)seq[mt][i] * V + col, __float_as_uint(z));
            }
    }
}

// Top-m of one sequence's row of zmax, one block per sequence: the m largest z > 0, best first, ties to the lower term
// id; terms padded with -1 and weights with 0; nnz = the number of z > 0 before the cut.  Exact selection on the bit
// patterns: a radix select (four 8-bit passes over the row, which is L2 resident) finds the value of rank
// min(m, nnz); everything above it is taken, and of its equals the lowest ids.  Where every equal is taken (the last
// pass counted them; the usual case, values being distinct) no order among them is needed and the row is read strided,
// as in the passes before; otherwise every thread owns a contiguous id range and a prefix sum over the threads' counts
// gives each equal its rank (uncoalesced and serial, for ties at the cut only).  The <= 512 survivors are sorted in LDS as
// (bits << 32 | ~id), a bitonic network over 512 slots.  w = (float) log1p((double) z), on the returned entries only.
constexpr int kSparseMaxM = 512;
__global__ __launch_bounds__(256) void k_vocab_topm(const unsigned* __restrict__ zmax, int V, int m, int32_t* __restrict__ terms,
                                                    float* __restrict__ weights, int32_t* __restrict__ nnz_out) {
    __shared__ unsigned hist[256], scan[256];
    __shared__ unsigned long long sel[kSparseMaxM];
    __shared__ unsigned sh_prefix, sh_remain, sh_cnt, sh_eq;
    const int tid = threadIdx.x;
    const unsigned* z = zmax + (size_t)blockIdx.x * V;
    if (tid == 0) sh_cnt = 0;
    for (int j = tid; j < kSparseMaxM; j += 256) sel[j] = 0ull;
    __syncthreads();
    unsigned cnt = 0;
    for (int i = tid; i < V; i += 256) cnt += z[i] != 0u;
    atomicAdd(&sh_cnt, cnt);
    __syncthreads();
    const int nnz = (int)sh_cnt;
    const int want = min(m, nnz);
    __syncthreads();
    if (want > 0) {   // (uniform over the block)
        unsigned prefix = 0, mask = 0, remain = (unsigned)want;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < V; i += 256) {
                const unsigned k = z[i];
                if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0;
                for (int bin = 255; bin >= 0; --bin) {
                    const unsigned h = hist[bin];
                    if (cum + h >= remain) {
                        sh_prefix = prefix | ((unsigned)bin << shift);
                        sh_remain = remain - cum;
                        sh_eq = h;   // (after the last pass: the entries equal to the threshold)
                        break;
                    }
                    cum += h;
                }
                sh_cnt = 0;
            }
            __syncthreads();
            prefix = sh_prefix;
            remain = sh_remain;
            mask |= 255u << shift;
            __syncthreads();
        }
        const unsigned thr = prefix;              // the value of rank `want` (> 0, since want <= nnz)
        const unsigned ngt = (unsigned)want - remain;   // entries above it; `remain` of its equals are taken
        if (sh_eq == remain) {   // (uniform) every equal is taken: ngt + remain = want <= 512 entries, in any order
            for (int i = tid; i < V; i += 256) {
                const unsigned k = z[i];
                if (k >= thr) {
                    const unsigned pos = atomicAdd(&sh_cnt, 1u);
                    if (pos < (unsigned)kSparseMaxM) sel[pos] = ((unsigned long long)k << 32) | (0xFFFFFFFFu - (unsigned)i);
                }
            }
        } else {
            const int seg = (V + 255) / 256, lo = tid * seg, hi = min(lo + seg, V);
            unsigned eq = 0;
            for (int i = lo; i < hi; ++i) {
                const unsigned k = z[i];
                if (k > thr) {
                    const unsigned pos = atomicAdd(&sh_cnt, 1u);
                    if (pos < (unsigned)kSparseMaxM) sel[pos] = ((unsigned long long)k << 32) | (0xFFFFFFFFu - (unsigned)i);
                } else if (k == thr) {
                    ++eq;
                }
            }
            scan[tid] = eq;
            __syncthreads();
            unsigned rank = 0;
            for (int j = 0; j < tid; ++j) rank += scan[j];
            for (int i = lo; i < hi && rank < remain; ++i) {
                if (z[i] != thr) continue;
                sel[ngt + rank] = ((unsigned long long)thr << 32) | (0xFFFFFFFFu - (unsigned)i);
                ++rank;
            }
        }
        __syncthreads();
        for (int k = 2; k <= kSparseMaxM; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;
                const unsigned long long x = sel[i], y = sel[p];
                const bool down = (i & k) == 0;   // this run is sorted largest first
                if (down ? x < y : x > y) {
                    sel[i] = y;
                    sel[p] = x;
                }
                __syncthreads();
            }
        }
    }
    for (int j = tid; j < m; j += 256) {
        const unsigned long long s = sel[j];
        const bool ok = j < want;
        terms[(size_t)blockIdx.x * m + j] = ok ? (int32_t)(0xFFFFFFFFu - (unsigned)(s & 0xFFFFFFFFull)) : -1;
        weights[(size_t)blockIdx.x * m + j] = ok ? (float)log1p((double)__uint_as_float((unsigned)(s >> 32))) : 0.f;
    }
    if (tid == 0) nnz_out[blockIdx.x] = nnz;
}

// ---------------------------------------------------------------- weights
// [N][K] fp32 -> bf16 with the K order of the blocked activation layout (preblk_kpos): the weights of a GEMM whose A
// operand is a blocked tensor (FFN2 reading the blocked FFN1 output).
__global__ void k_f32_to_bf16_kperm(const float* __restrict__ in, bf16_t* __restrict__ out, size_t n, int K) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const size_t row = i / (size_t)K;
        const int k = (int)(i - row * (size_t)K);
        out[G8_BBLK ? preblk_elem((int)row, k, K) : row * (size_t)K + preblk_kpos(k)] = f2bf(in[i]);
    }
}

__global__ void k_f32_to_bf16(const float* __restrict__ in, bf16_t* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = f2bf(in[i]);
}

}  // namespace css
