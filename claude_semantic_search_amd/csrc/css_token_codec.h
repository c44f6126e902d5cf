// css_token_codec.h -- residual compression of the flat index's token matrices (ColBERTv2's codec): a token is stored
// as the id of its best centroid plus an nbits bucket per component for the residual, and MaxSim runs on the codes.
// Included by css_index.hip in front of css_tokens.h, whose kernels decode with the primitives here (it reuses v8bf,
// v4f, kWaves, kLexNoRow).  include/css_hip.h defines the codec in bits.
//
// Encode.  code = argmax_c dot(d, centroid_c), ties to the lower c, with the dot formed as k_maxsim forms its own (bf16
// operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16, K steps of 32 ascending); r_j = fp32(d_j) -
// fp32(centroid[code]_j); bucket_j = #{i : cutoffs[i] < r_j}.  Decode.  d'_j = bf16_rne(fp32(centroid[code]_j) +
// weights[bucket_j]).  NO renormalisation after decoding (ColBERTv2 has one): a float32 restatement in numpy gives the
// same bytes.
//
// Layout in HBM = the canonical one of the C ABI: codes uint16 [ntok]; res uint8 [ntok, RB], RB = P nbits / 8
// (4 .. 64 bytes, always a multiple of 4): component j's bucket in bits [nbits (j % (8 / nbits)), +nbits) of byte
// j nbits / 8.  The 8 components 32 ks + 8 g .. + 7 that lane (l & 15, g = l >> 4) feeds to the MFMA of K step ks are
// the nbits consecutive bytes nbits (4 ks + g) .. of the token, so a lane reads its fragment's buckets with ONE load
// of nbits bytes per K step and a tile of 16 tokens is the 16 RB contiguous bytes that its wave reads whole: no
// permutation between the canonical and the stored form.
//
// MaxSim on the codes is k_tok_scores<P, MT, NB> (css_tokens.h) with NB = nbits: its B fragment is decoded in registers
// by tok_decode1 below.  The weights of a kernel sit in registers (NB <= 2: selects) or in 16 floats of LDS (NB = 4:
// distinct banks).
#pragma once

typedef short tok_v8s __attribute__((ext_vector_type(8)));   // the 8 bf16 that a lane feeds to one K step

template <int NB>
__device__ __forceinline__ unsigned tok_res_load(const unsigned char* p) {   // NB bytes, zero extended; p is NB-aligned
    if constexpr (NB == 1) return __builtin_nontemporal_load(p);
    else if constexpr (NB == 2) return __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(p));
    else return __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p));
}
__device__ __forceinline__ float tok_bf2f(short h) { return __uint_as_float((unsigned)(unsigned short)h << 16); }
// the ONE decode: one fp32 addition, one rounding to nearest even
__device__ __forceinline__ __bf16 tok_decode1(short c, float w) { return (__bf16)(tok_bf2f(c) + w); }

// the weights of one kernel: the first four in registers (four scalars, not an array), all 16 in LDS for NB = 4
struct TokWeights {
    const float* wl;
    float w0, w1, w2, w3;
};
template <int NB>
__device__ __forceinline__ float tok_weight(unsigned b, const TokWeights& w) {
    // (read before the selects: a select between the struct's members would keep the struct in memory)
    const float w0 = w.w0, w1 = w.w1, w2 = w.w2, w3 = w.w3;
    if constexpr (NB == 1) return b ? w1 : w0;
    else if constexpr (NB == 2) {
        // The weight's BITS, picked by masks from the bucket's two bits: u0 at 0, u1 at 1, u2 at 2, u3 at 3.  The four
        // weights and their differences stay in SGPRs; selects would hold all four in VGPRs (a wave per SIMD in two
        // instantiations) and a nested ?: is compiled into branches or into selects depending on where it is inlined.
        const unsigned u0 = __float_as_uint(w0), u1 = __float_as_uint(w1), u2 = __float_as_uint(w2), u3 = __float_as_uint(w3);
        const unsigned m0 = 0u - (b & 1u), m1 = 0u - (b >> 1);
        return __uint_as_float(u0 ^ (m0 & (u0 ^ u1)) ^ (m1 & (u0 ^ u2)) ^ (m0 & m1 & (u0 ^ u1 ^ u2 ^ u3)));
    }
    else return w.wl[b];
}
// Staged at the top of a kernel by every thread of its block (NB = 4: with a block barrier) from the table of 16 floats
// (zeros behind 2^NB) into the block's 16 floats of LDS `wl`.  NB = 0, a raw store, has no table and reads nothing.
template <int NB>
__device__ __forceinline__ TokWeights tok_weights_stage(const float* __restrict__ wts, float* wl) {
    static_assert(NB == 0 || NB == 1 || NB == 2 || NB == 4, "bits of a bucket (0: the raw store)");
    TokWeights w = {wl, 0.f, 0.f, 0.f, 0.f};
    if constexpr (NB == 4) {
        if (threadIdx.x < 16) wl[threadIdx.x] = wts[threadIdx.x];
        __syncthreads();
    }
    if constexpr (NB != 0) w.w0 = wts[0], w.w1 = wts[1], w.w2 = wts[2], w.w3 = wts[3];
    return w;
}

// k_tok_encode<P>: a wave takes kEncTiles tiles of 16 tokens (A, in registers) against every tile of 16 centroids (B,
// read through the caches: every wave walks the table in the same order), so a centroid fragment feeds kEncTiles MFMAs.
// C/D: lane l holds centroid column 16 ct + (l & 15) for the tokens 4 (l >> 4) + i of each tile: a running
// (max, argmax) per lane with a strict >, so a lane keeps its lowest column; the 16 lanes of a row group are then
// combined with "larger, or equal and lower id", which is order-free: ties go to the lower centroid whatever the tile
// order.  Centroids beyond C inside the last tile enter -inf.  Then, per 8 components of a token: the subtraction, the
// bucket count and nbits bytes of packed buckets.  The wave parks its codes in its own LDS row between the two halves.
constexpr int kEncTiles = 4;

template <int P>
__global__ __launch_bounds__(64 * kWaves) void k_tok_encode(const unsigned short* __restrict__ tok, int64_t ntok,
                                                            const unsigned short* __restrict__ cent, int C, int nbits,
                                                            const float* __restrict__ cut,
                                                            unsigned short* __restrict__ codes,
                                                            unsigned char* __restrict__ res) {
    constexpr int KS = P / 32, TT = kEncTiles, CH = P / 8;
    __shared__ unsigned short scode[kWaves][16 * TT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const float ninf = -__builtin_inff();
    const int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * (16 * TT);
    if (base >= ntok) return;   // (wave uniform; no block barrier below)
    v8bf a[TT][KS];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int64_t t = min(base + 16 * tt + lr, ntok - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            a[tt][ks] = __builtin_bit_cast(v8bf, *reinterpret_cast<const uint4*>(tok + (size_t)t * P + 32 * ks + 8 * g));
    }
    float best[TT][4];
    int bidx[TT][4];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            best[tt][i] = ninf;
            bidx[tt][i] = 0;
        }
    for (int c0 = 0; c0 < C; c0 += 16) {
        const int cc = min(c0 + lr, C - 1);
        const bool ok = c0 + lr < C;
        v8bf b[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            b[ks] = __builtin_bit_cast(v8bf, *reinterpret_cast<const uint4*>(cent + (size_t)cc * P + 32 * ks + 8 * g));
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[tt][ks], b[ks], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = ok ? acc[i] : ninf;
                if (v > best[tt][i]) {
                    best[tt][i] = v;
                    bidx[tt][i] = c0 + lr;
                }
            }
        }
    }
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = best[tt][i];
            int c = bidx[tt][i];
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) {
                const float ov = __shfl_xor(v, x, 64);
                const int oc = __shfl_xor(c, x, 64);
                if (ov > v || (ov == v && oc < c)) {
                    v = ov;
                    c = oc;
                }
            }
            if (lr == 0) scode[wave][16 * tt + 4 * g + i] = (unsigned short)c;
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int64_t t0 = base + lane;
    if (t0 < ntok) codes[t0] = scode[wave][lane];
    const int ncut = (1 << nbits) - 1;
    const size_t RB = (size_t)CH * nbits;
    for (int c = lane; c < 16 * TT * CH; c += 64) {
        const int tl = c / CH, ch = c % CH;
        const int64_t t = base + tl;
        if (t >= ntok) break;   // (tl ascends with c)
        const unsigned code = scode[wave][tl];
        const tok_v8s d = *reinterpret_cast<const tok_v8s*>(tok + (size_t)t * P + 8 * ch);
        const tok_v8s cn = *reinterpret_cast<const tok_v8s*>(cent + (size_t)code * P + 8 * ch);
        unsigned bits = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = tok_bf2f(d[j]) - tok_bf2f(cn[j]);
            unsigned bk = 0u;
            for (int i = 0; i < ncut; ++i) bk += cut[i] < r ? 1u : 0u;
            bits |= bk << (nbits * j);
        }
        unsigned char* out = res + (size_t)t * RB + (size_t)ch * nbits;
        if (nbits == 1) *out = (unsigned char)bits;
        else if (nbits == 2) *reinterpret_cast<unsigned short*>(out) = (unsigned short)bits;
        else *reinterpret_cast<unsigned*>(out) = bits;
    }
}

// css_index_get_tokens on a compressed store: 8 components per thread, the decode of k_tok_scores on the codes.
__global__ __launch_bounds__(256) void k_tok_decode(const unsigned short* __restrict__ codes,
                                                    const unsigned char* __restrict__ res, int64_t ntok,
                                                    const unsigned short* __restrict__ cent, int P, int nbits,
                                                    const float* __restrict__ wts, unsigned short* __restrict__ out) {
    const int CH = P / 8;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = idx / CH;
    const int ch = (int)(idx % CH);
    if (t >= ntok) return;
    const unsigned char* rp = res + (size_t)t * CH * nbits + (size_t)ch * nbits;
    const unsigned bits = nbits == 1 ? *rp : nbits == 2 ? *reinterpret_cast<const unsigned short*>(rp) : *reinterpret_cast<const unsigned*>(rp);
    const tok_v8s cn = *reinterpret_cast<const tok_v8s*>(cent + (size_t)codes[t] * P + 8 * ch);
    v8bf d;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = tok_decode1(cn[j], wts[(bits >> (nbits * j)) & ((1u << nbits) - 1u)]);
    *reinterpret_cast<uint4*>(out + (size_t)t * P + 8 * ch) = __builtin_bit_cast(uint4, d);
}

// The mover of css_index_remove_rows, one wave per source row r < nlist: a kept row's tokens move to token noff[map[r]]
// of the new buffer (map[r] = the row's new number, kLexNoRow when it goes), in units of T, u units per token (uint4,
// P / 8: the raw tokens; uint16, 1: the codes; uint32, RB / 4 = 1 .. 16: the packed buckets of 4 to 64 bytes).
template <typename T>
__global__ __launch_bounds__(256) void k_tok_move_units(const T* __restrict__ src, const int64_t* __restrict__ off,
                                                        const uint32_t* __restrict__ map, const int64_t* __restrict__ noff,
                                                        int64_t nlist, int u, T* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= nlist) return;
    const uint32_t nr = map[r];
    if (nr == kLexNoRow) return;
    const int64_t s = off[r] * u, cnt = (off[r + 1] - off[r]) * u, d = noff[nr] * u;
    for (int64_t i = lane; i < cnt; i += 64) dst[d + i] = src[s + i];
}
