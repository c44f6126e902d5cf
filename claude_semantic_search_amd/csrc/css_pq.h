// css_pq.h -- the product-quantized row store: a row of d components is M = d / 8 bytes, byte m the number of one of
// the 256 bf16 centroids of sub-quantizer m (include/css_hip.h has the definition "in bits").  Included by
// css_index.hip inside its anonymous namespace, behind css_fde.h (it reuses kWaves, v8bf and v4f).
//
// The store.  Codes are kept K-STEP MAJOR: plane ks (one K step of 32 components = 4 sub-quantizers) holds, row after
// row, the 4 bytes code[row][4 ks .. 4 ks + 3]: codes[(ks * cap + row) * 4 + (m & 3)], cap = the capacity in rows (a
// multiple of 64).  A row is still exactly M bytes.  The caller's row-major [n][M] form exists only at the ABI
// (k_pq_codes_in / k_pq_codes_out).  Row-major would let a wave touch 16 bytes of every row's cache line per codebook
// slice and fetch the line again for the next slice (M / 16 times over); plane-major makes every K step of a wave a
// contiguous run that is read once.
//
// k_pq_scores<G>: scores of up to 16 queries over a tile of 256 G rows per block, all of d, no look-up table.
//   MFMA     v_mfma_f32_16x16x32_bf16, A = the 16 queries (lane (l & 15, g = l >> 4) holds components 32 ks + 8 g .. + 7
//            of query l & 15, read per slice from `qf`, which k_pq_queries wrote in exactly that order), B = 16 rows.
//            Lane (l & 15, g) of B supplies components 32 ks + 8 g .. + 7 of its row: sub-quantizer 4 ks + g, whole.  So
//            the B fragment is ONE ds_read_b128 of codebook[4 ks + g][code] from LDS: the decode is the operand fetch.
//   rows     a wave owns G groups of 64 consecutive rows; in a group lane l & 15 = c stands for rows 4 c .. 4 c + 3, one
//            per tile j = 0 .. 3, so ONE 16-byte load per lane and K step (the 4 code bytes of 4 rows; 256 contiguous
//            bytes per wave, the four lane groups g read the same bytes) feeds four MFMAs: byte g of word j is the code.
//   slices   the block walks d in slices of 16 sub-quantizers = 4 K steps = 64 KB of codebook, brought into LDS by
//            LDS-DMA (global_load_lds_dwordx4, 1 KB per wave instruction, the slice is contiguous in memory).  One
//            slice is resident per block; two blocks fit a CU's 160 KB, so one block's DMA runs under the other's MFMAs.
//            The 16 G accumulator registers of a lane stay live across all slices: one fp32 accumulator per (query,
//            row) runs over the whole of d with the K steps ascending.
//   output   lane (c, g) ends with D[query 4 g + i][row 4 c + j]: col[query][row], -inf where the row is masked.
//   traffic  a block reads the whole codebook (4096 M bytes, from L2) for 256 G rows of M bytes: 16 / G codebook bytes
//            per code byte (2 at G = 8, where a pass over 10 M rows is 4900 blocks; 16 at G = 1, taken only when there
//            are too few rows to give every CU two larger tiles).
//   LDS      the gathers are data dependent.  A ds_read_b128 serves 16 lanes per step, 16 bytes each = all 64 banks
//            once when the 16 codes are distinct mod 16 (or equal: a broadcast).  Codes of the 16 rows (same
//            sub-quantizer) that differ but agree mod 16 collide: worst case 16-way, for uniform codes the expected
//            maximum is about 3.  Any placement of 256 entries of 16 bytes puts 16 of them on each bank quad, so a
//            swizzle only renames the worst case; the layout is the plain one.
//
// k_pq_encode: fp32 VALU, the definition's chain.  A block stages 8 sub-quantizers (bf16, 4 KB + 16 bytes apart so that
// two sub-quantizers of a wave sit on different banks); thread (sub-quantizer t >> 5, rows t & 31 + 32 i, i < 4) keeps
// its four sub-vectors in registers and walks the 256 centroids once, every centroid one broadcast ds_read_b128.
#pragma once

constexpr int kPqSliceSubq = 16;                          // sub-quantizers of a codebook slice of k_pq_scores
constexpr int kPqSliceBytes = kPqSliceSubq * 256 * 16;    // 64 KB
constexpr int kPqEncSubq = 8, kPqEncRows = 128, kPqEncStride = 4096 + 16;

struct PqScoreArgs {
    const unsigned char* __restrict__ codes;   // [M / 4][cap][4]
    const uint4* __restrict__ cb;              // [M][256] centroids of 8 bf16
    const uint4* __restrict__ qf;              // [M / 4][64]: the A fragments of this pass's 16 queries
    const uint32_t* __restrict__ mask;         // allow bits or null
    float* __restrict__ col;                   // [nq][n]
    int64_t n, cap;
    int M, nq;                                 // nq: the queries of this pass, 1 .. 16
};

template <int G>
__global__ __launch_bounds__(64 * kWaves) void k_pq_scores(const PqScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [16][256] centroids of 16 bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int KS = a.M / 4, nsl = (KS + 3) / 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kWaves + wave) * (64 * G);   // the wave's first row

    v4f acc[G][4];
#pragma unroll
    for (int gr = 0; gr < G; ++gr)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[gr][j] = v4f{0.f, 0.f, 0.f, 0.f};

    for (int sl = 0; sl < nsl; ++sl) {
        const int nk = min(4, KS - 4 * sl);   // K steps of this slice (the last one may be partial)
        __syncthreads();                      // every wave is done with the slice before
        const char* src = reinterpret_cast<const char*>(a.cb) + (size_t)sl * kPqSliceBytes + lane * 16;
        for (int ch = wave; ch < 16 * nk; ch += kWaves)   // 1 KB per instruction: lane l's 16 bytes land at + 16 l
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + ch * 1024),
                                             (__attribute__((address_space(3))) void*)(smem + ch * 1024), 16, 0, 0);
        v8bf qa[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            qa[ks] = __builtin_bit_cast(v8bf, ks < nk ? a.qf[(size_t)(4 * sl + ks) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

#pragma unroll
        for (int gr = 0; gr < G; ++gr) {
            const int64_t base = row0 + 64 * gr;
            if (base >= a.n) break;   // (wave uniform)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks >= nk) break;  // (block uniform)
                // rows base + 4 c .. + 3 of plane 4 sl + ks: within the allocation whenever the first is a row (cap is a
                // multiple of 64); bytes of rows past n are whatever they are and their scores are not stored
                uint4 cw = make_uint4(0u, 0u, 0u, 0u);
                if (base + 4 * c < a.n)
                    cw = *reinterpret_cast<const uint4*>(a.codes + ((size_t)(4 * sl + ks) * a.cap + base + 4 * c) * 4);
                const char* sub = smem + (4 * ks + g) * 4096;
                const unsigned w[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned code = (w[j] >> (8 * g)) & 0xFFu;
                    const v8bf cent = __builtin_bit_cast(v8bf, *reinterpret_cast<const uint4*>(sub + code * 16));
                    acc[gr][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], cent, acc[gr][j], 0, 0, 0);
                }
            }
        }
    }

    // lane (c, g): D[query 4 g + i][row base + 4 c + j]
#pragma unroll
    for (int gr = 0; gr < G; ++gr) {
        const int64_t base = row0 + 64 * gr + 4 * c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = base + j;
            if (row >= a.n) continue;
            const bool off = a.mask != nullptr && !((a.mask[row >> 5] >> (row & 31)) & 1u);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * g + i < a.nq) a.col[(size_t)(4 * g + i) * (size_t)a.n + row] = off ? -INFINITY : acc[gr][j][i];
        }
    }
}

__device__ __forceinline__ unsigned pq_bf16_rne(float x) {   // finite x
    const unsigned u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// fp32 queries [nq][d] -> qf [passes][d / 32][64] uint4: per pass of 16 queries the A fragments, bf16 RNE; the queries
// beyond nq are zero
__global__ void k_pq_queries(const float* __restrict__ q, int nq, int d, uint4* __restrict__ qf, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63), c = lane & 15, g = lane >> 4, KS = d / 32;
    const int ks = (int)((t >> 6) % KS), query = (int)((t >> 6) / KS) * 16 + c;
    unsigned h[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (query < nq) {
        const float* x = q + (size_t)query * d + 32 * ks + 8 * g;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = pq_bf16_rne(x[j]);
    }
    qf[t] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
}

// code[m] = argmin_c sum_j (x[8 m + j] - cent[m][c][j])^2 of rows x [n][8 M] into the store at rows first .. first + n - 1:
// fp32, one rounding per operation, j ascending, ties to the lower c.  Grid (ceil(n / 128), ceil(M / 8)).
__global__ __launch_bounds__(256) void k_pq_encode(const float* __restrict__ x, int64_t n, int M, const uint4* __restrict__ cb,
                                                   unsigned char* __restrict__ codes, int64_t cap, int64_t first) {
    __shared__ __attribute__((aligned(16))) char stage[kPqEncSubq * kPqEncStride];
    const int tid = threadIdx.x, m0 = blockIdx.y * kPqEncSubq, nm = min(kPqEncSubq, M - m0);
    for (int i = tid; i < nm * 256; i += 256)
        *reinterpret_cast<uint4*>(stage + (i >> 8) * kPqEncStride + (i & 255) * 16) = cb[(size_t)m0 * 256 + i];
    __syncthreads();
    const int sq = tid >> 5, m = m0 + sq;
    if (sq >= nm) return;
    const int64_t r0 = (int64_t)blockIdx.x * kPqEncRows + (tid & 31);
    float xv[4][8], best[4];
    int bi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = r0 + 32 * i;
        best[i] = INFINITY;
        bi[i] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[i][j] = 0.f;
        if (row < n) {
            const float4 lo = *reinterpret_cast<const float4*>(x + (size_t)row * 8 * M + 8 * m);
            const float4 hi = *reinterpret_cast<const float4*>(x + (size_t)row * 8 * M + 8 * m + 4);
            xv[i][0] = lo.x, xv[i][1] = lo.y, xv[i][2] = lo.z, xv[i][3] = lo.w;
            xv[i][4] = hi.x, xv[i][5] = hi.y, xv[i][6] = hi.z, xv[i][7] = hi.w;
        }
    }
    const char* sub = stage + sq * kPqEncStride;
    for (int ce = 0; ce < 256; ++ce) {
        const uint4 v = *reinterpret_cast<const uint4*>(sub + ce * 16);
        const float cf[8] = {__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16),
                             __uint_as_float(v.y & 0xFFFF0000u), __uint_as_float(v.z << 16), __uint_as_float(v.z & 0xFFFF0000u),
                             __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xFFFF0000u)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = __fsub_rn(xv[i][j], cf[j]);
                s = __fadd_rn(s, __fmul_rn(t, t));
            }
            if (s < best[i]) {
                best[i] = s;
                bi[i] = ce;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = r0 + 32 * i;
        if (row < n) codes[((size_t)(m >> 2) * cap + first + row) * 4 + (m & 3)] = (unsigned char)bi[i];
    }
}

// the caller's row-major codes [n][M] into the store at rows first .. (IN), or rows first .. of the store out (!IN)
template <bool IN>
__global__ void k_pq_codes_move(unsigned char* __restrict__ flat, int64_t n, int M, unsigned char* __restrict__ codes, int64_t cap,
                                int64_t first) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * M) return;
    const int64_t row = t / M;
    const int m = (int)(t % M);
    unsigned char* at = codes + ((size_t)(m >> 2) * cap + first + row) * 4 + (m & 3);
    if (IN) *at = flat[t];
    else flat[t] = *at;
}

// rows first .. first + n - 1 of the store as fp32 [n][8 M]: the centroids widened; one thread per (row, sub-quantizer)
__global__ void k_pq_decode(const unsigned char* __restrict__ codes, int64_t cap, int64_t first, int64_t n, int M,
                            const uint4* __restrict__ cb, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * M) return;
    const int64_t row = t / M;
    const int m = (int)(t % M);
    const unsigned code = codes[((size_t)(m >> 2) * cap + first + row) * 4 + (m & 3)];
    const uint4 v = cb[(size_t)m * 256 + code];
    float4* o = reinterpret_cast<float4*>(out + (size_t)t * 8);
    o[0] = make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xFFFF0000u));
    o[1] = make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xFFFF0000u), __uint_as_float(v.w << 16),
                       __uint_as_float(v.w & 0xFFFF0000u));
}
