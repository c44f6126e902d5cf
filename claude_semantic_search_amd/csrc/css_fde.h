// css_fde.h -- MUVERA fixed-dimensional encodings: a token matrix [m, P] bf16 becomes ONE fp32 row of
// dim = reps * 2^k_sim * d_proj whose inner product with a query's row estimates the MaxSim score (include/css_hip.h
// has the definition "in bits").  Included by css_index.hip inside its anonymous namespace, behind css_tokens.h (it
// reuses kWaves, v8bf, v4f and tok_v8s).
//
// k_fde<P, NBT> (NBT = the 16-bucket tiles of a repetition: 1 up to k_sim = 4, 2 at k_sim = 5, 4 at k_sim = 6).
// Persistent blocks of kWaves waves; block b takes the contiguous run of matrices [b per, (b + 1) per).  A matrix is
// staged in LDS row-major in chunks of kFdeChunk tokens (rows of 2 P + 32 bytes, the tail up to a multiple of 32 rows
// zero); the four waves share the staged chunk and wave w OWNS repetitions w, w + 4, ...: everything of a repetition
// -- sketch, bucket sums, counts, fill, projection, division, store -- happens in one wave, so there is no cross-wave
// order, no atomics and the bits do not depend on the grid or the batch.  A matrix of at most kFdeChunk tokens is
// staged once for all repetitions; a longer one is staged again per group of four repetitions (from L2).
//
// Per repetition r and K step of 32 tokens:
//   sketch   2 tiles x P / 32 v_mfma_f32_16x16x32_bf16: A = 16 token rows (ds_read_b128 from the chunk), B = the
//            repetition's planes as 16 columns (columns >= k_sim are zero) in fragment order, read once per repetition
//            from `planes_f`.  Lane l then holds the dots of plane l & 15 with tokens 4 (l >> 4) + i; its bit
//            (dot > 0) << (l & 15) is OR-ed over the 16 lanes of its group by DPP, and lane 16 g + i writes the bucket
//            byte of token 4 g + i into the wave's own LDS table [512] (0xFF beyond the matrix's end: no bucket).
//   sums     Y^T [P x B] += X^T [P x 32] . OneHot [32 x B]: the X^T fragments come from the SAME row-major chunk through
//            ds_read_b64_tr_b16 (lane 4 q + c of a 16-lane group addresses token row + q, components 4 c .. 4 c + 3 of the
//            16-component tile and receives tokens row .. row + 3 of component (lane & 15)); the one-hot fragment is
//            formed in registers from 8 bucket bytes (one ds_read_b64).  P / 16 * NBT accumulator tiles (64 VGPRs at
//            P = 128, B = 32): lane l holds Y[bucket 16 bt + (l & 15)][component 16 pt + 4 (l >> 4) + i].
//            The counts are integer sums of the one-hot compares, reduced over the four lane groups at the end.
// At the end of the matrix, per repetition: (documents) the empty buckets take the token of least Hamming distance,
// ties to the lowest token (an integer argmin over the bucket bytes, the row re-read from global memory); the
// projection out[b][j] = sum_p Y[b][p] proj[j][p] runs on v_mfma_f32_16x16x4_f32 with the ACCUMULATORS as the A operand
// as they stand (K step (pt, i) contracts components 16 pt + 4 g + i, g = 0 .. 3) and `proj_f`, the fp32 copy of proj
// in exactly that order, as B: no data moves between the two products.  Then one IEEE division by the count
// (documents) and the store: a wave writes its repetition's contiguous [B * d_proj] slice in 64-byte runs.
//
// LDS: (2 P + 32) * kFdeChunk + kWaves * 512 bytes = 38 912 at P = 128: at most four blocks per CU; the launch asks
// the runtime how many are resident and makes the grid that.
#pragma once

constexpr int kFdeChunk = 128;      // tokens of a staged chunk
constexpr int kFdeMaxTokens = 512;  // CSS_MAX_ROW_TOKEN_VECTORS: the bucket table of a wave

typedef short fde_v4s __attribute__((ext_vector_type(4)));

struct FdeArgs {
    const int64_t* __restrict__ off;             // [n + 1]
    const unsigned short* __restrict__ tok;      // [off[n]][P]
    const uint4* __restrict__ planes_f;          // [R][P / 32][64]: the B fragments of a repetition's planes
    const float4* __restrict__ proj_f;           // [R][d_proj / 16][P / 16][64]: proj as the projection's B operands
    float* __restrict__ out;                     // [n][R * B * d_proj]
    unsigned char* __restrict__ buckets;         // [off[n]][R] or null
    int64_t n;
    int k_sim, d_proj, reps, is_query;
};

// OR over each group of 16 consecutive lanes (the four DPP steps of row16_allsum)
__device__ __forceinline__ int fde_row16_or(int v) {
    v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
    return v;
}

template <int P, int NBT>
__global__ __launch_bounds__(64 * kWaves) void k_fde(const FdeArgs a) {
    constexpr int KS = P / 32, PT = P / 16, STRIDE = 2 * P + 32;
    __shared__ __attribute__((aligned(16))) char stage[kFdeChunk * STRIDE];
    __shared__ __attribute__((aligned(16))) unsigned char wbuck[kWaves][kFdeMaxTokens];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
    const int B = 1 << a.k_sim, JT = a.d_proj / 16, R = a.reps;
    const int64_t dim = (int64_t)R * B * a.d_proj;
    const int64_t per = (a.n + gridDim.x - 1) / gridDim.x;
    const int64_t d0 = (int64_t)blockIdx.x * per, d1 = min(a.n, d0 + per);
    unsigned char* wb = wbuck[wave];
    // the transposed reads' lane offset: token row + (lr >> 2), components 4 (lr & 3) .. + 3 of a 16-component tile
    const int trlane = (8 * g + (lr >> 2)) * STRIDE + 8 * (lr & 3);

    for (int64_t doc = d0; doc < d1; ++doc) {
        const int64_t beg = a.off[doc];
        // (the host form has checked the lengths; device offsets are the caller's, and the table holds kFdeMaxTokens)
        const int m = (int)min((int64_t)kFdeMaxTokens, a.off[doc + 1] - beg);
        float* orow = a.out + doc * dim;
        if (m <= 0) {   // a matrix without tokens: a row of zeros
            for (int64_t i = tid; i < dim; i += 64 * kWaves) orow[i] = 0.f;
            continue;
        }
        const int nch = (m + kFdeChunk - 1) / kFdeChunk;
        for (int rg = 0; rg * kWaves < R; ++rg) {
            const int r = rg * kWaves + wave;
            const bool active = r < R;
            v4f acc[PT][NBT];
            int cnt[NBT];
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) {
                cnt[bt] = 0;
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) acc[pt][bt] = v4f{0.f, 0.f, 0.f, 0.f};
            }
            v8bf pl[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                pl[ks] = __builtin_bit_cast(v8bf, active ? a.planes_f[((size_t)r * KS + ks) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u));

            for (int ch = 0; ch < nch; ++ch) {
                const int c0 = ch * kFdeChunk, cn = min(kFdeChunk, m - c0), rows = (cn + 31) & ~31;
                if (nch > 1 || rg == 0) {   // (block uniform)
                    __syncthreads();        // every wave is done with the chunk before
                    for (int i = tid; i < rows * (P / 8); i += 64 * kWaves) {
                        const int row = i / (P / 8), pc = i % (P / 8);
                        uint4 v = make_uint4(0u, 0u, 0u, 0u);
                        if (row < cn) v = *reinterpret_cast<const uint4*>(a.tok + ((size_t)beg + c0 + row) * P + 8 * pc);
                        *reinterpret_cast<uint4*>(stage + row * STRIDE + 16 * pc) = v;
                    }
                    __syncthreads();
                }
                if (!active) continue;
                for (int s = 0; s < rows / 32; ++s) {
                    // sketch: the bucket bytes of the step's 32 tokens
#pragma unroll
                    for (int tile = 0; tile < 2; ++tile) {
                        const char* arow = stage + (32 * s + 16 * tile + lr) * STRIDE + 16 * g;
                        v4f d = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks) {
                            const v8bf x = __builtin_bit_cast(v8bf, *reinterpret_cast<const uint4*>(arow + 64 * ks));
                            d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, pl[ks], d, 0, 0, 0);
                        }
                        // lane (plane lr, group g) holds the dots of tokens 4 g + i: its bit, OR-ed over the group's 16 lanes
                        int bk4[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) bk4[i] = fde_row16_or(d[i] > 0.f ? 1 << lr : 0);
                        if (lr < 4) {   // lane 16 g + i writes token 4 g + i of the tile
                            const int mine = lr == 0 ? bk4[0] : lr == 1 ? bk4[1] : lr == 2 ? bk4[2] : bk4[3];
                            const int t = c0 + 32 * s + 16 * tile + 4 * g + lr;   // token of the matrix
                            const unsigned bk = t < m ? (unsigned)mine & (unsigned)(B - 1) : 0xFFu;
                            wb[t] = (unsigned char)bk;
                            if (a.buckets != nullptr && t < m) a.buckets[((size_t)beg + t) * R + r] = (unsigned char)bk;
                        }
                    }
                    // (one wave writes and reads its own table: the LDS keeps a wave's accesses in order)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const uint2 bw = *reinterpret_cast<const uint2*>(wb + c0 + 32 * s + 8 * g);
                    tok_v8s oh[NBT];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int bk = (int)(((j < 4 ? bw.x : bw.y) >> (8 * (j & 3))) & 0xFFu);
#pragma unroll
                        for (int bt = 0; bt < NBT; ++bt) {
                            // 1 where the byte is this lane's bucket, in integer arithmetic: a compare per (j, bt) would
                            // hold 8 NBT lane masks in scalar registers and spill them
                            const int hit = (int)((unsigned)((bk ^ (16 * bt + lr)) - 1) >> 31);
                            oh[bt][j] = (short)(hit * 0x3F80);   // bf16 1.0
                            cnt[bt] += hit;
                        }
                    }
                    // sums: Y^T += X^T . OneHot
                    const char* xrow = stage + 32 * s * STRIDE + trlane;
#pragma unroll
                    for (int pt = 0; pt < PT; ++pt) {
                        const fde_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((fde_v4s __attribute__((address_space(3)))*)(xrow + 32 * pt));
                        const fde_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((fde_v4s __attribute__((address_space(3)))*)(xrow + 32 * pt + 4 * STRIDE));
                        // (whole-vector shuffle + bit cast, as the attention kernel takes its transposed reads)
                        const tok_v8s both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                        const v8bf xt = __builtin_bit_cast(v8bf, both);
#pragma unroll
                        for (int bt = 0; bt < NBT; ++bt)
                            acc[pt][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xt, __builtin_bit_cast(v8bf, oh[bt]), acc[pt][bt], 0, 0, 0);
                    }
                }
            }
            if (!active) continue;

            // counts of bucket 16 bt + lr: the four lane groups' shares
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) {
                cnt[bt] += __shfl_xor(cnt[bt], 16);
                cnt[bt] += __shfl_xor(cnt[bt], 32);
            }
            if (!a.is_query) {
                // one tile of 16 buckets at a time: a single lane mask is live across the argmin loop
                const unsigned* wb32 = reinterpret_cast<const unsigned*>(wb);
#pragma unroll
                for (int bt = 0; bt < NBT; ++bt) {
                    const bool empty = cnt[bt] == 0 && 16 * bt + lr < B;
                    if (__ballot(empty) == 0ull) continue;
                    // key = distance << 16 | token: the least key is the nearest token, ties to the lowest
                    unsigned best = 0xFFFFFFFFu;
                    for (int w = g; 4 * w < m; w += 4) {   // (group g takes the words g, g + 4, ...)
                        const unsigned u = wb32[w];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const unsigned bk = (u >> (8 * q)) & 0xFFu;   // (0xFF beyond the end: distance >= 2, and token 4 w exists)
                            const unsigned key = (unsigned)__popc(bk ^ (unsigned)(16 * bt + lr)) << 16 | (unsigned)(4 * w + q);
                            best = min(best, bk == 0xFFu ? 0xFFFFFFFFu : key);
                        }
                    }
                    best = min(best, (unsigned)__shfl_xor((int)best, 16));
                    best = min(best, (unsigned)__shfl_xor((int)best, 32));
                    if (empty) {
                        const unsigned short* x = a.tok + ((size_t)beg + (best & 0xFFFFu)) * P + 4 * g;
#pragma unroll
                        for (int pt = 0; pt < PT; ++pt) {
                            const uint2 v = *reinterpret_cast<const uint2*>(x + 16 * pt);
                            acc[pt][bt] = v4f{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u),
                                              __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u)};
                        }
                        cnt[bt] = 1;
                    }
                }
            }
            // projection, division, store: lane l gets out[bucket 16 bt + 4 g + i][16 jt + lr]
            float* oslice = orow + (size_t)r * B * a.d_proj;
#pragma unroll
            for (int bt = 0; bt < NBT; ++bt) {
                float den[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) den[i] = (float)__shfl(cnt[bt], 4 * g + i);
                for (int jt = 0; jt < JT; ++jt) {
                    const float4* pf = a.proj_f + (((size_t)r * JT + jt) * PT) * 64 + lane;
                    v4f o = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int pt = 0; pt < PT; ++pt) {
                        const float4 w = pf[pt * 64];
                        o = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[pt][bt][0], w.x, o, 0, 0, 0);
                        o = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[pt][bt][1], w.y, o, 0, 0, 0);
                        o = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[pt][bt][2], w.z, o, 0, 0, 0);
                        o = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[pt][bt][3], w.w, o, 0, 0, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int b = 16 * bt + 4 * g + i;
                        if (b < B) {
                            // an empty bucket of a query (and only that) has count 0: its sums are 0 and stay undivided
                            const float v = a.is_query ? o[i] : __fdiv_rn(o[i], den[i]);
                            oslice[(size_t)b * a.d_proj + 16 * jt + lr] = v;
                        }
                    }
                }
            }
        }
    }
}
