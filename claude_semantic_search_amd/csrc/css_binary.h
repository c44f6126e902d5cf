// css_binary.h -- the binary row store: a row of d components is d bits, bit i = (x[i] > 0), and the distance of two rows
// is the Hamming distance of their codes (include/css_hip.h has the definition "in bits").  Included by css_index.hip
// inside its anonymous namespace, behind css_pq.h.
//
// The store.  Codes are kept in WORD PLANES: plane w holds, row after row, the 32-bit word w of every row (bit b of the
// word = component 32 w + b), codes[w * cap + row], cap = the capacity in rows (a multiple of 64).  The caller's
// row-major bytes (np.packbits: component 8 j + b is bit 7 - b of byte j) exist only at the ABI: read as a
// little-endian word, reversing the bits within each byte (k_bin_codes_move) gives the plane word and back.  A lane
// that stands for 4 consecutive rows loads ONE uint4 per plane; a wave instruction then reads 1 KB contiguous = 256 rows.
// A pass's queries lie in the same layout ([W][capq], capq a multiple of 16), so word w of 16 queries is one 64-byte run
// at a wave-uniform address: scalar loads.
//
// k_bin_encode: a wave reads 64 consecutive floats of a row coalesced; ONE ballot of x > 0 is 64 code bits = two plane
// words.  No LDS, no per-thread bit loops.  Rows and float queries alike.
//
// k_bin_topk<NQ>: scan and selection in one kernel; no [nq][n] column ever exists.
//   parts    every WAVE owns one contiguous, ascending range of rows (a multiple of 256) and walks it in steps of 256
//            rows: lane l stands for rows base + 4 l .. + 3.  Waves never talk: no block barrier anywhere.
//   scan     per step and plane one uint4 load per lane, and per query 4 x (v_xor, v_bcnt accumulate) against the
//            query word in a scalar register, into 4 NQ integer accumulators.  NQ = 1 / 4 / 16 is the query count class.
//   select   a wave keeps per query ONE ascending list of k keys in LDS, key = distance << 32 | row: the order of the
//            keys IS the order of the answer (smaller distance, then lower id), so the list's last key is the
//            threshold and a row enters iff key < threshold.  Per step and query every lane puts forward the best of
//            its 4 rows and ONE ballot finds the hits; they are inserted one by one (the ballot is taken again under
//            the new threshold after every insert, so the first step does not pop 256 rows of which k survive).  The
//            k smallest keys of a set do not depend on the order they were offered in: the list is exact whatever the
//            walk.  After warm-up a step costs a query one LDS broadcast, a compare and a ballot.
//   output   the lists as one part, keys[part][query][k], padded with kBinPad.
//
// k_bin_merge: one block per query picks the k smallest of the parts' keys, exactly and in parallel, where a serial
// list merge (k_merge_parts walks nparts x k candidates one wave_insert after the other) would cost more than the scan
// it follows -- a resident scan has a few thousand parts.  The distances are integers in [0, d]: a histogram in LDS
// gives T = the distance of the k-th best and the number of keys below it; every key below T is taken; of the keys AT T
// the lowest ids are wanted, and since part p's rows all precede part p + 1's and a part is sorted, those are the first
// ones in (part, position) order: a count per part chunk, one prefix sum, one more walk.  A bitonic sort of the <= 128
// taken keys orders them; the key splits into int32 distance and int64 id (INT32_MAX / -1 for padding).  The asymmetric
// scores (below) span 2^21 + 1 values: k_bin_merge<true> finds T in two digit rounds over the same histogram, and in
// three for the up to 29 bits of the scalar-quantized store's keys (css_sq.h).
#pragma once

constexpr unsigned long long kBinPad = ~0ull;
constexpr int kBinWavesPerBlock = 4;
constexpr int kBinMergeThreads = 1024;   // one block per query: its loads of the parts' keys are all the parallelism there is
constexpr int kBinAsymBias = 1 << 20;    // an asymmetric score s, |s| <= 128 * 8192, has the key high word kBinAsymBias - s
// k_bin_merge<true>: the bits below the first digit of high words in [0, top], 10 per further round; the first digit
// has at most 4097 values.  top = 2^21: 10 (2049 bins, then 1024); top < 2^29: 20 (at most 512 bins, then 1024 twice).
__host__ __device__ constexpr int bin_wide_shift(int top) {
    int bits = 0;
    while (top >> bits) ++bits;
    return bits <= 12 ? 0 : (bits - 12 + 9) / 10 * 10;
}
// its dynamic LDS in bins: the first round's, and the 1024 of a further round
__host__ __device__ constexpr int bin_wide_bins(int top) {
    const int shift = bin_wide_shift(top), first = (top >> shift) + 1;
    return shift && first < 1024 ? 1024 : first;
}
constexpr int kBinWideBins = bin_wide_bins(2 * kBinAsymBias);
typedef const __attribute__((address_space(4))) unsigned* bin_const_words;

// bit b of the byte at every byte position <-> bit 7 - b: packbits bytes (as a little-endian word) <-> plane word
__device__ __forceinline__ unsigned bin_flip_bytes(unsigned v) { return __builtin_bswap32(__brev(v)); }

// fp32 rows x [n][d] -> plane words at rows first .. first + n - 1 of codes [d / 32][cap].  One wave per (row, chunk of
// 64 components), grid-stride over the n * ceil(d / 64) chunks.
__global__ __launch_bounds__(256) void k_bin_encode(const float* __restrict__ x, int64_t n, int d, unsigned* __restrict__ codes,
                                                    int64_t cap, int64_t first) {
    const int lane = threadIdx.x & 63, W = d / 32, C = (d + 63) / 64;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6), total = n * C;
    for (int64_t t = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += nwaves) {
        const int64_t row = t / C;
        const int c = (int)(t - row * C), i = 64 * c + lane;
        // x > 0 on the bits, so that denormals count whatever the wave's float mode: 0.0, -0.0 and NaN give 0
        const int u = i < d ? __float_as_int(x[(size_t)row * d + i]) : 0;
        const unsigned long long bits = __ballot(u > 0 && u <= 0x7F800000);
        if (lane == 0) codes[(size_t)(2 * c) * cap + first + row] = (unsigned)bits;
        if (lane == 1 && 2 * c + 1 < W) codes[(size_t)(2 * c + 1) * cap + first + row] = (unsigned)(bits >> 32);
    }
}

// the caller's row-major codes flat [n][W] (words of 4 packbits bytes) into the planes at rows first .. (IN), or rows
// first .. of the planes out (!IN); one thread per word, consecutive threads on consecutive rows of a plane
template <bool IN>
__global__ void k_bin_codes_move(unsigned* __restrict__ flat, int64_t n, int W, unsigned* __restrict__ codes, int64_t cap,
                                 int64_t first) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * W) return;
    const int64_t w = t / n, row = t - w * n;
    unsigned* at = codes + (size_t)w * cap + first + row;
    if (IN) *at = bin_flip_bytes(flat[(size_t)row * W + w]);
    else flat[(size_t)row * W + w] = bin_flip_bytes(*at);
}

struct BinTopkArgs {
    const unsigned* __restrict__ codes;      // [W][cap]
    const unsigned* __restrict__ qc;         // [W][capq], this pass's queries at q0 .. q0 + 15 of every plane
    const uint32_t* __restrict__ mask;       // allow bits or null
    unsigned long long* __restrict__ keys;   // [nwaves][nq][k]
    int64_t n, cap, per;                     // per: the rows of a wave's range, a multiple of 256
    int W, capq, q0, nq, k, nwaves;          // nq: the queries of this pass, 1 .. NQ
};

// `key` (wave uniform) into the ascending list L[0 .. k): every lane holds slots lane and lane + 64; all reads precede
// the writes (one wave, in step).  The caller knows key < L[k - 1].
__device__ __forceinline__ void bin_list_insert(unsigned long long* L, int k, unsigned long long key, int lane) {
    const int p0 = lane, p1 = lane + 64;
    const unsigned long long a0 = p0 < k ? L[p0] : kBinPad, b0 = p0 > 0 && p0 < k ? L[p0 - 1] : 0ull;
    const unsigned long long a1 = p1 < k ? L[p1] : kBinPad, b1 = p1 < k ? L[p1 - 1] : 0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // slot p keeps its key while that is below `key`, takes `key` where the slot before is below it (or p = 0), and the
    // slot before's key from there on
    if (p0 < k && !(a0 < key)) L[p0] = (p0 == 0 || b0 < key) ? key : b0;
    if (p1 < k && !(a1 < key)) L[p1] = b1 < key ? key : b1;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// The lane's rows row4 .. row4 + R - 1 at distances h[0 .. R) (`ok`: which of them may enter) offered to the list Lq
// (R = 4 in the Hamming scan, 16 in the asymmetric one).  Every
// lane puts forward its best pending row (the smallest distance, the lower row among equals); ONE ballot against the
// threshold finds the lanes with a hit -- after warm-up there is none and the wave moves on; otherwise the lowest such
// lane's row goes in and the ballot is taken again under the new threshold.
template <int R>
__device__ __forceinline__ void bin_offer(unsigned long long* Lq, int k, const int (&h)[R], unsigned row4, unsigned ok, int bits,
                                          int lane) {
    for (;;) {
        unsigned best = 0xFFFFFFFFu, bj = 0u;
#pragma unroll
        for (unsigned j = 0; j < (unsigned)R; ++j) {
            const unsigned hj = (ok >> j) & 1u ? (unsigned)h[j] : 0xFFFFFFFFu;
            if (hj < best) best = hj, bj = j;
        }
        const unsigned long long thr = Lq[k - 1];   // one address: a broadcast
        const bool hit = ok != 0u && ((unsigned long long)best << 32 | (row4 + bj)) < thr;
        if (__ballot(hit) == 0ull) return;
        // the smallest distance among the hits, bit by bit from the top with ballots alone (no LDS, no lane exchange):
        // its lowest lane holds the wave's smallest pending key, so a step inserts no row that a later row of the same
        // step would push out again -- the first step of a range makes k inserts, not k (1 + ln(256 / k))
        unsigned m = 0u;
        for (int b = bits - 1; b >= 0; --b)
            if (__ballot(hit && (best >> b) == (m >> b)) == 0ull) m |= 1u << b;
        const int src = __builtin_ctzll(__ballot(hit && best == m));
        const unsigned long long key = (unsigned long long)(unsigned)__shfl((int)best, src) << 32 | (unsigned)__shfl((int)(row4 + bj), src);
        bin_list_insert(Lq, k, key, lane);
        if (lane == src) ok &= ~(1u << bj);
    }
}

template <int NQ>
__global__ __launch_bounds__(64 * kBinWavesPerBlock) void k_bin_topk(const BinTopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long bin_lists[];   // [waves of the block][nq][k]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.k;
    const int part = blockIdx.x * kBinWavesPerBlock + wave;
    if (part >= a.nwaves) return;   // (no barrier below)
    unsigned long long* L = bin_lists + (size_t)wave * a.nq * k;
    for (int i = lane; i < a.nq * k; i += 64) L[i] = kBinPad;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int64_t lo = (int64_t)part * a.per, hi = min(a.n, lo + a.per);
    const int bits = 32 - __builtin_clz((unsigned)a.W * 32u);   // a distance is at most d = 32 W
    // the pass's query words through the constant address space: nothing writes them while the kernel runs, and a load at
    // a wave-uniform address from there is a scalar load
    const bin_const_words qc = (bin_const_words)(a.qc + a.q0);
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t row4 = base + 4 * lane;   // a multiple of 4: with row4 < n <= cap the uint4 lies within the plane
        const bool in = row4 < hi;
        int acc[NQ][4];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0;
        const unsigned* cp = a.codes + row4;
#pragma unroll NQ == 16 ? 2 : 4
        for (int w = 0; w < a.W; ++w) {
            const uint4 cw = in ? *reinterpret_cast<const uint4*>(cp + (size_t)w * a.cap) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const unsigned qw = qc[(size_t)w * a.capq + q];   // wave uniform: a scalar load (NQ words in a run)
                acc[q][0] += __popc(cw.x ^ qw);
                acc[q][1] += __popc(cw.y ^ qw);
                acc[q][2] += __popc(cw.z ^ qw);
                acc[q][3] += __popc(cw.w ^ qw);
            }
        }
        // the 4 allow bits of the lane's rows sit in one mask word (row4 is a multiple of 4); rows past the range: none
        unsigned ok = 0u;
        if (in) {
            const int64_t left = hi - row4;
            ok = left >= 4 ? 0xFu : (1u << left) - 1u;
            if (a.mask != nullptr) ok &= a.mask[row4 >> 5] >> (row4 & 31);
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q < a.nq) {   // (wave uniform)
                bin_offer(L + (size_t)q * k, k, acc[q], (unsigned)row4, ok, bits, lane);
            }
    }
    unsigned long long* out = a.keys + (size_t)part * a.nq * k;
    for (int i = lane; i < a.nq * k; i += 64) out[i] = L[i];
}

// exclusive prefix of `mine` over the block's threads through `buf` [kBinMergeThreads]
__device__ __forceinline__ unsigned bin_block_prefix(unsigned* buf, unsigned mine, int tid) {
    __syncthreads();   // (buf may still be read from the call before)
    buf[tid] = mine;
    __syncthreads();
    unsigned ex = 0u;
    for (int t = 0; t < tid; ++t) ex += buf[t];
    return ex;
}

// The bin of hist [nb] at which the running count reaches `want`, and the count below it, into *sT / *sBelow (left as
// they are when the bins hold fewer than `want`); every thread owns a run of bins.  Ends with a barrier.
__device__ __forceinline__ void bin_hist_kth(const unsigned* hist, int nb, unsigned* pre, unsigned want, int tid, unsigned* sT,
                                             unsigned* sBelow) {
    const int per = (nb + kBinMergeThreads - 1) / kBinMergeThreads, b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    unsigned mine = 0u;
    for (int b = b0; b < b1; ++b) mine += hist[b];
    unsigned c = bin_block_prefix(pre, mine, tid);
    if (c < want && c + mine >= want)   // (exactly one thread, if any)
        for (int b = b0; b < b1; ++b) {
            if (c + hist[b] >= want) {
                *sT = (unsigned)b, *sBelow = c;
                break;
            }
            c += hist[b];
        }
    __syncthreads();
}

// keys [nparts][nq][k] -> D / I [k] of query blockIdx.x: the k smallest keys, ascending.  Part p's rows all precede
// part p + 1's.  `top` is the largest high word a key can have.  !WIDE (Hamming: top = d): one histogram of top + 1 bins.
// WIDE (scores, high word = bias - score in [0, top]): the threshold in digit rounds over the high word from the top,
// the bits above bin_wide_shift(top) first, then 10 bits per round among the keys that share the upper digits of the
// k-th (top = 2^21: 2049 bins, then 1024); D is bias - the high word and the padding INT32_MIN.  Dynamic LDS:
// (WIDE ? bin_wide_bins(top) : top + 1) bins.
template <bool WIDE>
__global__ __launch_bounds__(kBinMergeThreads) void k_bin_merge(const unsigned long long* __restrict__ keys, int nparts, int nq, int k,
                                                                int top, int bias, int32_t* __restrict__ D, int64_t* __restrict__ I) {
    extern __shared__ unsigned bin_hist[];
    __shared__ unsigned pre[kBinMergeThreads];
    __shared__ unsigned long long sel[CSS_KERNEL_MAX_K];
    __shared__ unsigned sT, sBelow, sT2, sBelow2, sCnt;
    const int tid = threadIdx.x, q = blockIdx.x;
    const unsigned long long* kq = keys + (size_t)q * k;       // part p, entry j: kq[p * stride + j]
    const size_t stride = (size_t)nq * k;
    const int shift = WIDE ? bin_wide_shift(top) : 0, nb = (top >> shift) + 1;
    for (int i = tid; i < nb; i += kBinMergeThreads) bin_hist[i] = 0u;
    if (tid < CSS_KERNEL_MAX_K) sel[tid] = kBinPad;
    if (tid == 0) sT = (unsigned)nb, sBelow = 0u, sT2 = 0u, sBelow2 = 0u, sCnt = 0u;   // fewer than k keys in all: everything is "below"
    __syncthreads();
    const int total = nparts * k;
    for (int e = tid; e < total; e += kBinMergeThreads) {
        const int p = e / k, j = e - p * k;
        const unsigned long long key = kq[(size_t)p * stride + j];
        if (key != kBinPad) atomicAdd(&bin_hist[(unsigned)(key >> 32) >> shift], 1u);
    }
    __syncthreads();
    // T = the first distance at which the running count reaches k
    bin_hist_kth(bin_hist, nb, pre, (unsigned)k, tid, &sT, &sBelow);
    const bool found = sT < (unsigned)nb;
    unsigned T = found ? sT : 0xFFFFFFFFu, below = sBelow;
    if (WIDE && found)   // (block uniform) the next digit, among the keys whose upper digits are T
        for (int s = shift - 10; s >= 0; s -= 10) {
            for (int i = tid; i < 1024; i += kBinMergeThreads) bin_hist[i] = 0u;
            __syncthreads();
            for (int e = tid; e < total; e += kBinMergeThreads) {
                const int p = e / k, j = e - p * k;
                const unsigned long long key = kq[(size_t)p * stride + j];
                if (key != kBinPad && (unsigned)(key >> 32) >> (s + 10) == T) atomicAdd(&bin_hist[(unsigned)(key >> 32) >> s & 1023u], 1u);
            }
            __syncthreads();
            bin_hist_kth(bin_hist, 1024, pre, (unsigned)k - below, tid, &sT2, &sBelow2);
            T = T << 10 | sT2, below += sBelow2;
        }
    const unsigned need = found ? (unsigned)k - below : 0u;
    // every key below T, in any order, into sel[0 .. below)
    for (int e = tid; e < total; e += kBinMergeThreads) {
        const int p = e / k, j = e - p * k;
        const unsigned long long key = kq[(size_t)p * stride + j];
        if (key != kBinPad && (unsigned)(key >> 32) < T) sel[atomicAdd(&sCnt, 1u)] = key;
    }
    // the first `need` keys at T in (part, position) order into sel[below .. k): every thread owns a run of parts
    if (need) {   // (block uniform)
        const int np = (nparts + kBinMergeThreads - 1) / kBinMergeThreads, p0 = min(nparts, tid * np), p1 = min(nparts, p0 + np);
        unsigned mine = 0u;
        for (int p = p0; p < p1; ++p)
            for (int j = 0; j < k; ++j) {
                const unsigned h = (unsigned)(kq[(size_t)p * stride + j] >> 32);   // (padding: 0xFFFFFFFF > T)
                if (h > T) break;   // a part is sorted
                mine += h == T;
            }
        unsigned r = bin_block_prefix(pre, mine, tid);
        for (int p = p0; p < p1 && r < need; ++p)
            for (int j = 0; j < k && r < need; ++j) {
                const unsigned long long key = kq[(size_t)p * stride + j];
                const unsigned h = (unsigned)(key >> 32);
                if (h > T) break;
                if (h == T) sel[below + r++] = key;
            }
    }
    __syncthreads();
    // bitonic sort of sel[0 .. 128) ascending (padding last)
    for (int size = 2; size <= CSS_KERNEL_MAX_K; size <<= 1)
        for (int s = size >> 1; s > 0; s >>= 1) {
            if (tid < CSS_KERNEL_MAX_K / 2) {
                const int lo = 2 * tid - (tid & (s - 1)), hi = lo + s;
                const unsigned long long x = sel[lo], y = sel[hi];
                if ((x > y) == ((lo & size) == 0)) sel[lo] = y, sel[hi] = x;
            }
            __syncthreads();
        }
    if (tid < k) {
        const unsigned long long key = sel[tid];
        const int32_t hw = (int32_t)(key >> 32);
        D[(size_t)q * k + tid] = key == kBinPad ? (WIDE ? INT32_MIN : INT32_MAX) : WIDE ? bias - hw : hw;
        I[(size_t)q * k + tid] = key == kBinPad ? (int64_t)-1 : (int64_t)(key & 0xFFFFFFFFull);
    }
}

// the answer of a search of an empty store (`pad`: INT32_MAX for distances, INT32_MIN for scores)
__global__ void k_bin_pad(int32_t* __restrict__ D, int64_t* __restrict__ I, int64_t total, int32_t pad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    D[t] = pad;
    I[t] = -1;
}

// ------------------------------------------------------------------ asymmetric scoring: int8 queries against the bit codes
// s(q, r) = sum_i q_i (2 b_i - 1), the query at int8 and the row as it lies in the planes (include/css_hip.h).  It is a GEMM
// with one operand stored as bits, so it runs on v_mfma_i32_16x16x64_i8: the rows are the M side, decoded to 0 / 1 bytes ONCE
// per row and K step (not once per row and query), the pass's 16 queries are the N side, and the kernel accumulates
// t = sum_i q_i b_i; s = 2 t - sum_i q_i is applied per query in the epilogue.
//
// The tile.  A wave step covers 64 rows x 16 queries.  Lane (m = l & 15, g = l >> 4) loads ONE uint4 of plane 4 T + g at
// rows base + 4 m .. + 3 (256 contiguous bytes per plane, four planes per wave instruction).  Word j of the four is the A
// operand of row tile j (M index m = row base + 4 m + j), and feeds two K steps h = 0, 1.  A dot product does not care
// about the order of K, so the lane takes the 16 bits that are cheapest to spread: VGPR i of K step h is
// (word >> (4 h + i)) & 0x01010101, i.e. byte b holds bit 4 h + i + 8 b -- two VALU instructions per 4 bytes, 15 per word.
// k_bin_asym_prep lays the queries out to match: the B operand of K step (T, h) holds in lane (n, g), VGPR i, byte b the
// component 32 (4 T + g) + 4 h + i + 8 b of query n.  The MFMA leaves lane (n, G) with tile j's rows 4 G + r, r = 0 .. 3:
// over the four tiles the 16 CONSECUTIVE rows base + 16 G + 4 r + j of ONE query, the shape bin_offer works on.
//
// Queries: up to d = 1024 the pass's fragments stay in registers (16 uint4 = 64 VGPRs); above that the block stages them
// in LDS once (16 d bytes) and every K step reads its fragment from there (QLDS).
//
// Selection: as in k_bin_topk, per wave and query one ascending list of k keys in LDS, key = (2^20 - s) << 32 | row, so
// that the larger score and then the lower id come first.  Per step every lane compares the best of its 16 rows with ITS
// query's threshold and one ballot finds the queries with a hit (after warm-up: none); only those run bin_offer, their
// four lanes putting rows forward.  No block barrier in the scan.
struct BinAsymArgs {
    const unsigned* __restrict__ codes;      // [W][cap]
    const uint4* __restrict__ qf;            // this pass's query fragments [2 ceil(W / 4)][64]
    const int* __restrict__ qsum;            // this pass's sum_i q_i [16]
    const uint32_t* __restrict__ mask;       // allow bits or null
    unsigned long long* __restrict__ keys;   // [nwaves][nq][k]
    int64_t n, cap, per;                     // per: the rows of a wave's range, a multiple of 64
    int W, nq, k, nwaves;                    // nq: the queries of this pass, 1 .. 16
};

// fp32 (F32) or int8 queries [nq][d] -> fragments qf [capq / 16][2 ceil(W / 4)][64] uint4 and sums qsum [capq]; one wave
// per query slot, the slots past nq give zeros.  F32: a = max |q_i| (on the bits: |x| orders like its pattern), the query
// is all zeros if a is below the smallest normal, else q8_i = rint((q_i / a) * 127), the division and the product each
// rounded once (numpy float32 says the same; a denormal quotient gives 0 flushed or not).
template <bool F32>
__global__ __launch_bounds__(256) void k_bin_asym_prep(const void* __restrict__ q, int nq, int capq, int d, uint4* __restrict__ qf,
                                                       int* __restrict__ qsum) {
    const int lane = threadIdx.x & 63, qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= capq) return;
    const int nT = (d / 32 + 3) / 4, n = qi & 15;
    const float* qx = static_cast<const float*>(q) + (size_t)qi * d;
    const signed char* q8 = static_cast<const signed char*>(q) + (size_t)qi * d;
    float a = 0.f;
    if (F32 && qi < nq) {
        int top = 0;
        for (int i = lane; i < d; i += 64) top = max(top, __float_as_int(qx[i]) & 0x7FFFFFFF);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o));
        a = top >= 0x00800000 ? __int_as_float(top) : 0.f;
    }
    unsigned* out = reinterpret_cast<unsigned*>(qf + (size_t)(qi >> 4) * 2 * nT * 64);
    int sum = 0;
    // word o of the query's share of the fragments: K step t = 2 T + h, lane group g, VGPR i
    for (int o = lane; o < 32 * nT; o += 64) {
        const int i = o & 3, g = (o >> 2) & 3, t = o >> 4;
        unsigned word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = 32 * (4 * (t >> 1) + g) + 4 * (t & 1) + i + 8 * b;
            int v = 0;
            if (qi < nq && c < d) {
                if (F32) v = a > 0.f ? (int)rintf(__fmul_rn(__fdiv_rn(qx[c], a), 127.f)) : 0;
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

typedef int bin_v4i __attribute__((ext_vector_type(4)));

// one plane group: the lane's four words against the K steps' fragments b0, b1, into the four row tiles
__device__ __forceinline__ void bin_asym_step(const uint4 cw, const bin_v4i b0, const bin_v4i b1, bin_v4i (&acc)[4]) {
    const unsigned w[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        constexpr unsigned M = 0x01010101u;
        const bin_v4i a0{(int)(w[j] & M), (int)(w[j] >> 1 & M), (int)(w[j] >> 2 & M), (int)(w[j] >> 3 & M)};
        const bin_v4i a1{(int)(w[j] >> 4 & M), (int)(w[j] >> 5 & M), (int)(w[j] >> 6 & M), (int)(w[j] >> 7 & M)};
        acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, acc[j], 0, 0, 0);
    }
}

template <bool QLDS>
__global__ __launch_bounds__(64 * kBinWavesPerBlock) void k_bin_asym_topk(const BinAsymArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long bin_lists[];   // (QLDS: the fragments, then) [waves][nq][k]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.k;
    const int nT = (a.W + 3) / 4, nqf = QLDS ? 2 * nT * 64 : 0;
    const bin_v4i* qs = reinterpret_cast<const bin_v4i*>(bin_lists);
    bin_v4i qr[QLDS ? 1 : 16];
    if (QLDS) {
        uint4* dst = reinterpret_cast<uint4*>(bin_lists);
        for (int i = threadIdx.x; i < nqf; i += blockDim.x) dst[i] = a.qf[i];
        __syncthreads();   // (the only barrier: before the scan, and before any wave leaves)
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint4 v = t < 2 * nT ? a.qf[t * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
            qr[t] = bin_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
    }
    const int part = blockIdx.x * (blockDim.x >> 6) + wave;
    if (part >= a.nwaves) return;
    unsigned long long* L = bin_lists + 2 * (size_t)nqf + (size_t)wave * a.nq * k;
    for (int i = lane; i < a.nq * k; i += 64) L[i] = kBinPad;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

    const int64_t lo = (int64_t)part * a.per, hi = min(a.n, lo + a.per);
    const int n = lane & 15, g = lane >> 4;
    const int qsum = n < a.nq ? a.qsum[n] : 0;
    const unsigned long long* Ln = L + (size_t)min(n, a.nq - 1) * k;
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t row4 = base + 4 * n;   // a multiple of 4: with row4 < n <= cap the uint4 lies within the plane
        const bool in = row4 < hi;
        const unsigned* cp = a.codes + (size_t)g * a.cap + row4;
        bin_v4i acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = bin_v4i{0, 0, 0, 0};
        if (QLDS) {
            for (int T = 0; T < nT; ++T) {
                const uint4 cw = in && 4 * T + g < a.W ? *reinterpret_cast<const uint4*>(cp + (size_t)4 * T * a.cap) : make_uint4(0u, 0u, 0u, 0u);
                bin_asym_step(cw, qs[(2 * T) * 64 + lane], qs[(2 * T + 1) * 64 + lane], acc);
            }
        } else {
#pragma unroll
            for (int T = 0; T < 8; ++T)
                if (T < nT) {   // (wave uniform; the fragments are indexed at compile time)
                    const uint4 cw = in && 4 * T + g < a.W ? *reinterpret_cast<const uint4*>(cp + (size_t)4 * T * a.cap) : make_uint4(0u, 0u, 0u, 0u);
                    bin_asym_step(cw, qr[QLDS ? 0 : 2 * T], qr[QLDS ? 0 : 2 * T + 1], acc);
                }
        }
        // the lane's 16 rows row16 .. + 15 of query n: tile j, register r is row row16 + 4 r + j.  Their allow bits sit
        // in one mask word (row16 is a multiple of 16); rows past the range and query slots past nq: none
        const int64_t row16 = base + 16 * g;
        int h[16];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[4 * r + j] = kBinAsymBias + qsum - 2 * acc[j][r];
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
            bin_offer(L + (size_t)q * k, k, h, (unsigned)row16, n == q ? ok : 0u, 22, lane);
        }
    }
    unsigned long long* out = a.keys + (size_t)part * a.nq * k;
    for (int i = lane; i < a.nq * k; i += 64) out[i] = L[i];
}
