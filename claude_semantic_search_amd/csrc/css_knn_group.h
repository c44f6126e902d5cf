// css_knn_group.h -- grouped search on the flat index: the best row of each of the k best groups.
// Included by css_index.hip (inside its anonymous namespace, after k_mask_clear and compact_slot).
//
// Every row carries an int32 group label (css_index::labels; negative = the row is a group of its own).  A grouped
// search is the ordinary ranked, masked search followed by a collapse: in a best-first list of the top kk rows the
// first occurrences of distinct labels ARE the best groups, each with its best row, and every group that is absent has
// its best row below entry kk.  So the scan kernels stay untouched; what is new is bandwidth-trivial:
//
//   k_collapse_groups   one wave per query: stable compaction of a pass's [kk] results to first occurrences, appended
//                       behind the groups the query already holds (ballot + prefix popcount per 64 entries, as
//                       k_drop_self), the new group count and an "exhausted" flag (the pass came back padded)
//   k_mask_drop_groups  in front of a further pass of ONE query: every row whose label is among the groups found so
//                       far leaves the query's exclusion bitmap.  One lane per row, coalesced 4-byte label loads,
//                       membership by binary search in the (at most 128) found labels sorted in LDS, and the wave64
//                       ballot IS two whole mask words: plain stores, no atomics.  4 B + 1/8 B per row
//   k_gather_labels     G[j][i] = label of row I[j][i] (after the final sort)
//   k_compact_labels    css_index_remove_rows: the label column follows the rows, out of place
#pragma once

// Pass results Ds / Is: [nqp, kk] best-first lists of queries q0 .. q0 + nqp - 1 (ids global, pads -1 at the tail).
// Dg / Ig / Lg: [nq, k] groups found so far (score, id and label of each group's best row); state[2q] of them are
// valid (zero in front of a query's first pass), state[2q + 1] is the exhausted flag.  labels null: every row is its
// own group.
__global__ __launch_bounds__(256) void k_collapse_groups(const float* __restrict__ Ds, const int64_t* __restrict__ Is,
                                                         const int32_t* __restrict__ labels, int64_t id_base, int64_t q0,
                                                         int64_t nqp, int kk, int k, float pad, float* __restrict__ Dg,
                                                         int64_t* __restrict__ Ig, int32_t* __restrict__ Lg,
                                                         int* __restrict__ state) {
    __shared__ int32_t lab[4][CSS_KERNEL_MAX_K];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    const bool live = j < nqp;   // (no early return: the block meets at the barrier)
    const float* Dj = Ds + (size_t)(live ? j : 0) * kk;
    const int64_t* Ij = Is + (size_t)(live ? j : 0) * kk;
    for (int c = lane; c < kk; c += 64) {
        const int64_t id = live ? Ij[c] : -1;
        lab[wave][c] = (id >= 0 && labels) ? labels[id - id_base] : -1;
    }
    __syncthreads();
    if (!live) return;
    const int64_t q = q0 + j;
    float* Do = Dg + (size_t)q * k;
    int64_t* Io = Ig + (size_t)q * k;
    int32_t* Lo = Lg + (size_t)q * k;
    int have = state[2 * q];
    for (int c0 = 0; c0 < kk; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < kk;
        const int64_t id = in ? Ij[c] : -1;
        const float s = in ? Dj[c] : pad;
        const int32_t l = in ? lab[wave][c] : -1;
        bool keep = id >= 0;
        if (keep && l >= 0)
            for (int e = 0; e < c; ++e) keep = keep && lab[wave][e] != l;   // first occurrence of its label
        const unsigned long long b = __ballot(keep);
        const int pos = have + __popcll(b & ((1ull << lane) - 1ull));
        if (keep && pos < k) {
            Do[pos] = s;
            Io[pos] = id;
            Lo[pos] = l;
        }
        have += __popcll(b);
    }
    have = min(have, k);
    for (int c = have + lane; c < k; c += 64) {
        Do[c] = pad;
        Io[c] = -1;
        Lo[c] = -1;
    }
    if (lane == 0) {
        state[2 * q] = have;
        state[2 * q + 1] = Ij[kk - 1] < 0 ? 1 : 0;   // fewer than kk allowed rows were left: nothing more to find
    }
}

// mask: ceil(n / 32) words, bit (r & 31) of word r >> 5.  found: the nfound (<= CSS_KERNEL_MAX_K) labels of the groups
// the query holds; negative entries (ungrouped rows) are skipped here, their rows are cleared by k_mask_clear.
// Grid-stride over 256-row tiles, so a block sorts the labels once for many tiles.
__global__ __launch_bounds__(256) void k_mask_drop_groups(uint32_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                          int64_t n, const int32_t* __restrict__ found,
                                                          const int* __restrict__ nfound_p) {
    __shared__ int32_t raw[CSS_KERNEL_MAX_K];
    __shared__ int32_t sorted[CSS_KERNEL_MAX_K];
    __shared__ int m_sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const int nfound = min(*nfound_p, CSS_KERNEL_MAX_K);
    if (tid < CSS_KERNEL_MAX_K) raw[tid] = tid < nfound ? found[tid] : -1;
    __syncthreads();
    if (tid < CSS_KERNEL_MAX_K) {   // rank sort of the distinct non-negative labels (LDS broadcast reads)
        const int32_t v = raw[tid];
        int rank = 0, m = 0;
        for (int e = 0; e < CSS_KERNEL_MAX_K; ++e) {
            const int32_t w = raw[e];
            m += w >= 0;
            rank += w >= 0 && w < v;
        }
        if (v >= 0) sorted[rank] = v;
        if (tid == 0) m_sh = m;
    }
    __syncthreads();
    const int m = m_sh;
    if (m == 0) return;
    const int64_t words = (n + 31) >> 5;
    const int64_t tiles = (n + 255) >> 8;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r = t * 256 + tid;
        const int32_t l = r < n ? labels[r] : -1;
        bool hit = false;
        if (l >= 0) {
            int lo = 0, hi = m;   // first position whose label is not below l
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sorted[mid] < l) lo = mid + 1;
                else hi = mid;
            }
            hit = lo < m && sorted[lo] == l;
        }
        const unsigned long long b = __ballot(hit);
        const int64_t w = (r - lane) >> 5;   // first of the wave's two words
        if (lane == 0 && (uint32_t)b != 0u && w < words) mask[w] &= ~(uint32_t)b;
        if (lane == 32 && (uint32_t)(b >> 32) != 0u && w + 1 < words) mask[w + 1] &= ~(uint32_t)(b >> 32);
    }
}

__global__ void k_gather_labels(const int64_t* __restrict__ I, const int32_t* __restrict__ labels, int64_t id_base,
                                int64_t n, int32_t* __restrict__ G) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = I[i];
    G[i] = (id >= 0 && labels) ? labels[id - id_base] : -1;
}

// One lane per row of a window (bits / pre as k_compact_rows has them): dst is ANOTHER buffer, so nothing overlaps.
__global__ __launch_bounds__(256) void k_compact_labels(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre,
                                                        int64_t n, const int32_t* __restrict__ src, int32_t* __restrict__ dst) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t o = compact_slot(bits, pre, r);
    if (o >= 0) dst[o] = src[r];
}
