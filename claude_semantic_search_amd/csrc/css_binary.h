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
// taken keys orders them; the key splits into int32 distance and int64 id (INT32_MAX / -1 for padding).
#pragma once

constexpr unsigned long long kBinPad = ~0ull;
constexpr int kBinWavesPerBlock = 4;
constexpr int kBinMergeThreads = 1024;   // one block per query: its loads of the parts' keys are all the parallelism there is
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

// The lane's rows row4 .. row4 + 3 at distances h[0 .. 3] (`ok`: which of them may enter) offered to the list Lq.  Every
// lane puts forward its best pending row (the smallest distance, the lower row among equals); ONE ballot against the
// threshold finds the lanes with a hit -- after warm-up there is none and the wave moves on; otherwise the lowest such
// lane's row goes in and the ballot is taken again under the new threshold.
__device__ __forceinline__ void bin_offer(unsigned long long* Lq, int k, const int (&h)[4], unsigned row4, unsigned ok, int bits,
                                          int lane) {
    for (;;) {
        unsigned best = 0xFFFFFFFFu, bj = 0u;
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
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

// keys [nparts][nq][k] -> D / I [k] of query blockIdx.x: the k smallest keys, ascending.  Part p's rows all precede
// part p + 1's.  Dynamic LDS: d + 1 histogram bins.
__global__ __launch_bounds__(kBinMergeThreads) void k_bin_merge(const unsigned long long* __restrict__ keys, int nparts, int nq, int k,
                                                                int d, int32_t* __restrict__ D, int64_t* __restrict__ I) {
    extern __shared__ unsigned bin_hist[];   // [d + 1]
    __shared__ unsigned pre[kBinMergeThreads];
    __shared__ unsigned long long sel[CSS_KERNEL_MAX_K];
    __shared__ unsigned sT, sBelow, sCnt;
    const int tid = threadIdx.x, q = blockIdx.x;
    const unsigned long long* kq = keys + (size_t)q * k;       // part p, entry j: kq[p * stride + j]
    const size_t stride = (size_t)nq * k;
    for (int i = tid; i <= d; i += kBinMergeThreads) bin_hist[i] = 0u;
    if (tid < CSS_KERNEL_MAX_K) sel[tid] = kBinPad;
    if (tid == 0) sT = (unsigned)d + 1u, sBelow = 0u, sCnt = 0u;   // fewer than k keys in all: everything is "below"
    __syncthreads();
    const int total = nparts * k;
    for (int e = tid; e < total; e += kBinMergeThreads) {
        const int p = e / k, j = e - p * k;
        const unsigned long long key = kq[(size_t)p * stride + j];
        if (key != kBinPad) atomicAdd(&bin_hist[(unsigned)(key >> 32)], 1u);
    }
    __syncthreads();
    // T = the first distance at which the running count reaches k; every thread owns a run of bins
    {
        const int nb = (d + 1 + kBinMergeThreads - 1) / kBinMergeThreads, b0 = tid * nb, b1 = min(d + 1, b0 + nb);
        unsigned mine = 0u;
        for (int b = b0; b < b1; ++b) mine += bin_hist[b];
        unsigned c = bin_block_prefix(pre, mine, tid);
        if (c < (unsigned)k && c + mine >= (unsigned)k)   // (exactly one thread, if any)
            for (int b = b0; b < b1; ++b) {
                if (c + bin_hist[b] >= (unsigned)k) {
                    sT = (unsigned)b, sBelow = c;
                    break;
                }
                c += bin_hist[b];
            }
    }
    __syncthreads();
    const unsigned T = sT, below = sBelow, need = T <= (unsigned)d ? (unsigned)k - below : 0u;
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
        D[(size_t)q * k + tid] = key == kBinPad ? INT32_MAX : (int32_t)(key >> 32);
        I[(size_t)q * k + tid] = key == kBinPad ? (int64_t)-1 : (int64_t)(key & 0xFFFFFFFFull);
    }
}

// the answer of a search of an empty store
__global__ void k_bin_pad(int32_t* __restrict__ D, int64_t* __restrict__ I, int64_t total) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    D[t] = INT32_MAX;
    I[t] = -1;
}
