// css_sq.h -- the scalar-quantized row store: a row of d components is d codes of 8 or 4 bits, code i the level of
// x[i] on a per-component grid vmin[i] + c step[i], and a search ranks the rows by the integer sum_i q8_i c_i with the
// ranges folded into an int8 query (include/css_hip.h has the definition "in bits").  Included by css_index.hip inside
// its anonymous namespace, behind css_binary.h, whose selection (bin_list_insert, bin_offer<16>, the key form
// (bias - s) << 32 | row) and merge (k_bin_merge<true>) it uses.
//
// The store.  At the ABI a row is RB = d bits / 8 bytes, row-major; at 4 bits component 2 j is the low nibble of byte j.
// On the device the SAME bytes lie ROW-TILE-MAJOR, so that the scan reads them as MFMA A-fragments with no LDS and no
// transpose.  The granule is 16 consecutive ABI bytes of one row (16 components at 8 bits, 32 at 4), one uint4.  Rows go
// in groups of 64, a row's bytes in chunks of 64 (C = ceil(RB / 64) chunks; RB is a multiple of 16, so a granule lies in
// the row or past it), and granule (row, y) sits at uint4
//       (((row / 64) C + y / 4) 4 + row % 4) 64 + 16 (y % 4) + (row % 64) / 4:
// group, chunk c, tile j = row % 4, and within the tile's KB lane 16 g + m with g = y % 4, m = (row % 64) / 4.  A wave
// instruction of the scan loads ONE such KB (lane l its uint4 l), the 4 tiles of a chunk are 4 KB in a run and a group
// 4 C KB in a run.  A group never depends on the rows behind it: appending writes new granules and moves none, and
// growing is one copy of the bytes as they lie.  The capacity is whole groups; the granules past RB in the last chunk
// and the rows past ntotal in the last group hold nothing the scan uses (the first are loaded as zeros, the second are
// never offered).
//
// Why tile j holds rows 4 m + j and not 16 j + m: v_mfma_i32_16x16x64_i8 leaves lane (n, G) with the tile's rows
// M = 4 G + r, r = 0 .. 3, of query n; over the four tiles that is rows base + 16 G + 4 r + j, SIXTEEN CONSECUTIVE rows
// of one query per lane -- the shape bin_offer<16> works on, with the 16 allow bits in one mask word.
//
// The K order.  A dot product does not care about the order of K as long as both operands agree: lane (m, g), VGPR i,
// byte b of the A operand is ABI byte 64 c + 16 g + 4 i + b of the row, AS IT LIES.  At 8 bits that is component
// 64 c + 16 g + 4 i + b, and the codes go in as c - 128 (one v_xor per dword), 128 sum_i q8_i added per query in the
// epilogue.  At 4 bits a dword gives two operand dwords, v & 0x0F0F0F0F (components 128 c + 32 g + 8 i + 2 b) and
// (v >> 4) & 0x0F0F0F0F (the same + 1): 3 VALU per 8 operand bytes, two K steps per chunk.  k_sq_prep applies the
// permutation ONCE, to the query fragments.
//
// k_sq_topk<BITS, QLDS>: scan and selection in one kernel, no score column.  Every wave owns one contiguous ascending
// range of whole groups and walks it 64 rows x 16 queries at a time: per chunk four KB loads and 4 (8 bits) or 8 (4 bits)
// MFMAs into one accumulator per tile.  The pass's fragments stay in registers up to d = 1024 (16 uint4 = 64 VGPRs at
// either width); above, the block stages them in LDS once (16 d bytes, the only barrier, before the scan).  Selection is
// that of k_bin_asym_topk: per wave and query one ascending list of k keys in LDS, one ballot per step finds the queries
// with a hit.  bias = 128 L d bounds |s|, so the high word bias - s lies in [0, 2 bias] (< 2^29 at d = 8192, 8 bits).
#pragma once

constexpr int kSqRegFrags = 16;   // the query fragments (K steps of 64) that k_sq_topk<.., false> keeps in registers

// the uint4 of granule y of row `row` in a store of C chunks per row (above)
__device__ __forceinline__ size_t sq_at(int64_t row, int y, int C) {
    const int rr = (int)(row & 63);
    return (((size_t)(row >> 6) * C + (y >> 2)) * 4 + (rr & 3)) * 64 + 16 * (y & 3) + (rr >> 2);
}

// clamp(rintf((x - vmin) / step), 0, L), every operation rounded once (a NaN, which only the _dev forms let through: 0)
template <int BITS>
__device__ __forceinline__ unsigned sq_code(float x, float vmin, float step) {
    const float t = rintf(__fdiv_rn(__fsub_rn(x, vmin), step));
    return (unsigned)fminf(fmaxf(t, 0.f), (float)((1 << BITS) - 1));
}

// fp32 rows x [n][d] -> codes at rows first .. first + n - 1.  One thread per granule, grid-stride.
template <int BITS>
__global__ __launch_bounds__(256) void k_sq_encode(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ vmin,
                                                   const float* __restrict__ step, uint4* __restrict__ codes, int C, int64_t first) {
    constexpr int PER = 128 / BITS;   // the components of a granule
    const int G = d / PER;
    const int64_t total = n * G, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t row = t / G;
        const int y = (int)(t - row * G), c0 = PER * y;
        const float* xr = x + (size_t)row * d + c0;
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                unsigned v;
                if (BITS == 8) {
                    const int e = 4 * i + b;
                    v = sq_code<8>(xr[e], vmin[c0 + e], step[c0 + e]);
                } else {
                    const int e = 8 * i + 2 * b;
                    v = sq_code<4>(xr[e], vmin[c0 + e], step[c0 + e]) | sq_code<4>(xr[e + 1], vmin[c0 + e + 1], step[c0 + e + 1]) << 4;
                }
                w[i] |= v << (8 * b);
            }
        }
        codes[sq_at(first + row, y, C)] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// the caller's row-major codes flat [n][G] granules into the store at rows first .. (IN), or rows first .. of the store
// out (!IN); one thread per granule
template <bool IN>
__global__ void k_sq_codes_move(uint4* __restrict__ flat, int64_t n, int G, uint4* __restrict__ codes, int C, int64_t first) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * G) return;
    const int64_t row = t / G;
    uint4* at = codes + sq_at(first + row, (int)(t - row * G), C);
    if (IN) *at = flat[t];
    else flat[t] = *at;
}

// rows first .. first + n - 1 decoded to out [n][d]: fmaf(c, step, vmin), one rounding.  One thread per granule.
template <int BITS>
__global__ void k_sq_reconstruct(const uint4* __restrict__ codes, int C, int64_t first, int64_t n, int d, const float* __restrict__ vmin,
                                 const float* __restrict__ step, float* __restrict__ out) {
    constexpr int PER = 128 / BITS;
    const int G = d / PER;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * G) return;
    const int64_t row = t / G;
    const int y = (int)(t - row * G), c0 = PER * y;
    const uint4 v = codes[sq_at(first + row, y, C)];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    float* o = out + (size_t)row * d + c0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const unsigned c = BITS == 8 ? w[e >> 2] >> (8 * (e & 3)) & 0xFFu : w[e >> 3] >> (4 * (e & 7)) & 0xFu;
        o[e] = __fmaf_rn((float)c, step[c0 + e], vmin[c0 + e]);
    }
}

// fp32 (F32) or int8 queries [nq][d] -> fragments qf [capq / 16][nF][64] uint4 in the K order of the scan and sums qsum
// [capq]; one wave per query slot, the slots past nq give zeros.  nF = ceil(d / 64) at 8 bits, 2 ceil(d / 128) at 4.
// F32 folds the ranges in: w_i = q_i step_i (one rounding), a = max |w_i| (on the bits: |x| orders like its pattern), the
// query is all zeros if a is below the smallest normal, else q8_i = rint((w_i / a) * 127), the division and the product
// each rounded once -- k_bin_asym_prep's rule on w.  fp32 denormals are kept (the compiler's default for this target): a
// denormal w_i under a normal a counts.
template <bool F32>
__global__ __launch_bounds__(256) void k_sq_prep(const void* __restrict__ q, int nq, int capq, int d, int bits,
                                                 const float* __restrict__ step, uint4* __restrict__ qf, int* __restrict__ qsum) {
    const int lane = threadIdx.x & 63, qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= capq) return;
    const int nF = bits == 8 ? (d + 63) / 64 : 2 * ((d + 127) / 128), n = qi & 15;
    const float* qx = static_cast<const float*>(q) + (size_t)qi * d;
    const signed char* q8 = static_cast<const signed char*>(q) + (size_t)qi * d;
    float a = 0.f;
    if (F32 && qi < nq) {
        int top = 0;
        for (int i = lane; i < d; i += 64) top = max(top, __float_as_int(__fmul_rn(qx[i], step[i])) & 0x7FFFFFFF);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o));
        a = top >= 0x00800000 ? __int_as_float(top) : 0.f;
    }
    unsigned* out = reinterpret_cast<unsigned*>(qf + (size_t)(qi >> 4) * nF * 64);
    int sum = 0;
    // word o of the query's share of the fragments: K step t, lane group g, VGPR i
    for (int o = lane; o < 16 * nF; o += 64) {
        const int i = o & 3, g = (o >> 2) & 3, t = o >> 4;
        unsigned word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = bits == 8 ? 64 * t + 16 * g + 4 * i + b : 128 * (t >> 1) + 32 * g + 8 * i + 2 * b + (t & 1);
            int v = 0;
            if (qi < nq && c < d) {
                if (F32) v = a > 0.f ? (int)rintf(__fmul_rn(__fdiv_rn(__fmul_rn(qx[c], step[c]), a), 127.f)) : 0;
                else v = q8[c];
            }
            sum += v;
            word |= (unsigned)(v & 0xFF) << (8 * b);
        }
        out[((size_t)t * 64 + 16 * g + n) * 4 + i] = word;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) qsum[qi] = sum;
}

struct SqTopkArgs {
    const uint4* __restrict__ codes;         // [groups][C][4][64]
    const uint4* __restrict__ qf;            // this pass's query fragments [nF][64]
    const int* __restrict__ qsum;            // this pass's sum_i q8_i [16]
    const uint32_t* __restrict__ mask;       // allow bits or null
    unsigned long long* __restrict__ keys;   // [nwaves][nq][k]
    int64_t n, per;                          // per: the rows of a wave's range, a multiple of 64
    int C, rb, nq, k, nwaves;                // rb: the bytes of a row; nq: the queries of this pass, 1 .. 16
    int bias, kbits;                         // the key's high word is bias - s, below 2^kbits
};

// one chunk: the lane's granules of the four tiles (cp: tile 0's; `live`: within the row's bytes) against the chunk's
// fragment b0 (8 bits) or its low- and high-nibble fragments b0, b1 (4 bits), into the four tiles' accumulators
template <int BITS>
__device__ __forceinline__ void sq_chunk(const uint4* __restrict__ cp, bool live, const bin_v4i b0, const bin_v4i b1, bin_v4i (&acc)[4]) {
    uint4 cw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cw[j] = live ? cp[64 * j] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (BITS == 8) {
            constexpr unsigned X = 0x80808080u;   // c -> c - 128 as an int8
            const bin_v4i a0{(int)(cw[j].x ^ X), (int)(cw[j].y ^ X), (int)(cw[j].z ^ X), (int)(cw[j].w ^ X)};
            acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc[j], 0, 0, 0);
        } else {
            constexpr unsigned M = 0x0F0F0F0Fu;
            const bin_v4i a0{(int)(cw[j].x & M), (int)(cw[j].y & M), (int)(cw[j].z & M), (int)(cw[j].w & M)};
            const bin_v4i a1{(int)(cw[j].x >> 4 & M), (int)(cw[j].y >> 4 & M), (int)(cw[j].z >> 4 & M), (int)(cw[j].w >> 4 & M)};
            acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, acc[j], 0, 0, 0);
        }
    }
}

template <int BITS, bool QLDS>
__global__ __launch_bounds__(64 * kBinWavesPerBlock) void k_sq_topk(const SqTopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sq_lists[];   // (QLDS: the fragments, then) [waves][nq][k]
    constexpr int FPC = BITS == 8 ? 1 : 2;   // the fragments of a chunk
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.k;
    const int nF = FPC * a.C, nqf = QLDS ? nF * 64 : 0;
    const bin_v4i* qs = reinterpret_cast<const bin_v4i*>(sq_lists);
    bin_v4i qr[QLDS ? 1 : kSqRegFrags];
    if (QLDS) {
        uint4* dst = reinterpret_cast<uint4*>(sq_lists);
        for (int i = threadIdx.x; i < nqf; i += blockDim.x) dst[i] = a.qf[i];
        __syncthreads();   // (the only barrier: before the scan, and before any wave leaves)
    } else {
#pragma unroll
        for (int t = 0; t < kSqRegFrags; ++t) {
            const uint4 v = t < nF ? a.qf[t * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
            qr[t] = bin_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
    }
    const int part = blockIdx.x * (blockDim.x >> 6) + wave;
    if (part >= a.nwaves) return;
    unsigned long long* L = sq_lists + 2 * (size_t)nqf + (size_t)wave * a.nq * k;
    for (int i = lane; i < a.nq * k; i += 64) L[i] = kBinPad;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int64_t lo = (int64_t)part * a.per, hi = min(a.n, lo + a.per);
    const int n = lane & 15, g = lane >> 4;
    // the high word of a key is bias - s; at 8 bits s = acc + 128 sum_i q8_i (the codes went in as c - 128)
    const int hb = a.bias - (BITS == 8 && n < a.nq ? 128 * a.qsum[n] : 0);
    const unsigned long long* Ln = L + (size_t)min(n, a.nq - 1) * k;
    for (int64_t base = lo; base < hi; base += 64) {
        const uint4* cp = a.codes + (size_t)(base >> 6) * a.C * 256 + lane;   // the group is whole within the capacity
        bin_v4i acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = bin_v4i{0, 0, 0, 0};
        if (QLDS) {
            for (int c = 0; c < a.C; ++c)
                sq_chunk<BITS>(cp + (size_t)c * 256, 64 * c + 16 * g < a.rb, qs[FPC * c * 64 + lane], qs[(FPC * c + FPC - 1) * 64 + lane], acc);
        } else {
#pragma unroll
            for (int c = 0; c < kSqRegFrags / FPC; ++c)
                if (c < a.C)   // (wave uniform; the fragments are indexed at compile time)
                    sq_chunk<BITS>(cp + c * 256, 64 * c + 16 * g < a.rb, qr[QLDS ? 0 : FPC * c], qr[QLDS ? 0 : FPC * c + FPC - 1], acc);
        }
        // the lane's 16 rows row16 .. + 15 of query n: tile j, register r is row row16 + 4 r + j.  Their allow bits sit
        // in one mask word (row16 is a multiple of 16).  Rows past the range -- the last group's tail holds whatever
        // the memory held, and a zero code would beat every real row under a negative query -- and query slots past
        // nq: none
        const int64_t row16 = base + 16 * g;
        int h[16];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[4 * r + j] = hb - acc[j][r];
        unsigned ok = 0u;
        if (row16 < hi && n < a.nq) {
            const int64_t left = hi - row16;
            ok = left >= 16 ? 0xFFFFu : (1u << left) - 1u;
            if (a.mask != nullptr) ok &= a.mask[row16 >> 5] >> (row16 & 31);
        }
        unsigned best = 0xFFFFFFFFu;
#pragma unroll
        for (unsigned j = 0; j < 16; ++j)
            if ((ok >> j) & 1u) best = min(best, (unsigned)h[j]);
        // every lane against ITS query's threshold, on the high words alone: `<=` may send a query to bin_offer that then
        // finds no hit (a tie in score with a higher row), never the other way
        unsigned long long hits = __ballot(ok != 0u && best <= (unsigned)(Ln[k - 1] >> 32));
        unsigned qm = (unsigned)(hits | hits >> 16 | hits >> 32 | hits >> 48) & 0xFFFFu;
        while (qm) {   // (wave uniform)
            const int q = __builtin_ctz(qm);
            qm &= qm - 1u;
            bin_offer(L + (size_t)q * k, k, h, (unsigned)row16, n == q ? ok : 0u, a.kbits, lane);
        }
    }
    unsigned long long* out = a.keys + (size_t)part * a.nq * k;
    for (int i = lane; i < a.nq * k; i += 64) out[i] = L[i];
}
