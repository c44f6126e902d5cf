// css_sparse.h -- learned sparse vectors on the flat index: one (term, weight) list per row in HBM, the dot column of
// ONE query over all rows, and the exact top-k of that column.  Included by css_index.hip (inside its anonymous
// namespace, behind css_lexical.h: it reuses kWaves, kLexNoRow and wave_insert).
//
// Layout.  Row r < T (T = the leading rows that were given a vector) owns entries [off[r], off[r + 1]) of `ent`: 8 bytes
// per distinct term, the uint32 term in the low word and the bits of the float weight in the high word, ascending by
// term, so a lane loads one entry with one 8-byte load.  Rows >= T have no vector.  There is no df table and no length:
// a dot product needs no corpus statistics, so a shard's column equals the single index's by construction.
//
// k_sparse_scores.  The structure of k_lex_scores (css_lexical.h): a wave owns the entry span of ROWS consecutive rows
// and streams it with one entry per lane and LOADS loads in flight; an entry's term is looked up in the 4096-slot LDS
// byte table of the query terms (terms that share their low 12 bits are chained); the entry's row comes from a bisection
// in the wave's ROWS + 1 offsets; a match (row, j) writes the STORED WEIGHT into the wave's LDS table [ROWS][MQ] of
// floats.  A stored weight is > 0, so a zero slot means "absent" and there is no flag table.  Lane r < ROWS then sums row
// r in QUERY-TERM order in fp32 (include/css_hip.h has the definition) and the wave stores one coalesced segment of the
// column.  A row without a match gets `miss`: 0.0f for the hybrid search, -inf for the pure sparse search.
// The table rows are MQ + 1 dwords apart, an odd stride, so the lanes read distinct LDS banks.  Two instantiations,
// both 4 waves per block and 39 KB of LDS, four blocks per CU: <32, 4, 64, 4> for m <= 32 (64 rows per wave, 8.4 KB of
// table each) and <64, 4, 32, 4> for m <= 64 (32 rows per wave, 8.3 KB each).  A 64-row table of 64 terms is 16.6 KB per
// wave: four of them do not fit the 64 KB a block may declare, and the 2-wave block that does fit leaves 8 waves per CU
// and took 1.7 times as long (DESIGN.md 3.2n has the three measurements).
// Traffic: 8 E + 8 N bytes read, 4 N written.
//
// Two kernels, not one skeleton shared with k_lex_scores: the entry width (8 against 4 bytes), the table element (a
// float against a tf byte), the block shape and the epilogue all differ, and the BM25 column is checked bit for bit
// and timed as it stands; what the two would share is the 20-line streaming loop, at the price of a template over
// four traits around it.  A change to the loop of one is made to both.
//
// k_sparse_topk.  Block b takes the slice [b * slice, (b + 1) * slice) of the column; its four waves take the 64-row
// chunks of the slice in turn, skip -inf (no hit) and masked rows, and keep one best-first k-list each in LDS with
// wave_insert, the list code of the fp32 sweeps; wave 0 then folds the other three lists into its own and writes the
// block's part list (scores, global ids, -1 in empty slots), which merge_parts joins.  The comparator is total (larger
// value, then lower id), so the result does not depend on the geometry.
#pragma once

constexpr int kSparseTopkMinSlice = 4096;   // rows per block of k_sparse_topk at least ...
constexpr int kSparseTopkMaxParts = 32;     // ... and at most this many blocks (the part merge is one wave)

template <int MQ, int WAVES, int ROWS, int LOADS>
__global__ __launch_bounds__(64 * WAVES) void k_sparse_scores(const unsigned long long* __restrict__ ent,
                                                              const int64_t* __restrict__ off, int64_t nlist, int64_t ntotal,
                                                              const uint32_t* __restrict__ qterms,
                                                              const float* __restrict__ qweights, int m, float miss,
                                                              float* __restrict__ col) {
    constexpr int kStride = MQ + 1;
    __shared__ uint32_t slot_w[1024];   // 4096 byte slots
    __shared__ unsigned char nxt[MQ];
    __shared__ uint32_t qt[MQ];
    __shared__ float qw[MQ];
    __shared__ uint32_t roff[WAVES][ROWS + 1];
    __shared__ float tab[WAVES][ROWS * kStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* slot = reinterpret_cast<unsigned char*>(slot_w);
    for (int i = tid; i < 1024; i += 64 * WAVES) slot_w[i] = 0u;
    if (tid < MQ) {
        qt[tid] = tid < m ? qterms[tid] : 0u;
        qw[tid] = tid < m ? qweights[tid] : 0.f;
    }
    for (int i = lane; i < ROWS * kStride; i += 64) tab[wave][i] = 0.f;
    const int64_t base = ((int64_t)blockIdx.x * WAVES + wave) * ROWS;
    const int nrow = (int)std::min<int64_t>(std::max<int64_t>(nlist - base, 0), ROWS);   // rows of this wave with a vector
    int64_t s = 0;
    uint32_t mine = 0u, last = 0u;
    if (nrow > 0) {
        s = off[base];
        mine = (uint32_t)(off[base + std::min(lane, nrow)] - s);   // (a wave's span is at most 64 * 2^16 entries)
        last = (uint32_t)(off[base + nrow] - s);
    }
    if (lane < ROWS) roff[wave][lane] = mine;
    if (lane == 0) roff[wave][ROWS] = last;
    __syncthreads();
    if (tid == 0)   // chains in ascending j: built from the back, each term put in front of its slot
        for (int j = m - 1; j >= 0; --j) {
            const uint32_t hslot = qt[j] & 4095u;
            nxt[j] = slot[hslot];
            slot[hslot] = (unsigned char)(j + 1);
        }
    __syncthreads();

    const uint32_t span = last;
    const unsigned long long* e = ent + s;
    for (uint32_t i0 = 0; i0 < span; i0 += 64 * LOADS) {
        unsigned long long v[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const uint32_t idx = i0 + u * 64 + lane;
            v[u] = idx < span ? __builtin_nontemporal_load(e + idx) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const uint32_t idx = i0 + u * 64 + lane;
            const uint32_t term = (uint32_t)v[u];
            uint32_t at = idx < span ? slot[term & 4095u] : 0u;
            while (at != 0u) {
                const int j = (int)at - 1;
                if (qt[j] == term) {
                    int r = 0;   // the last row whose first entry is at or below idx
#pragma unroll
                    for (int step = ROWS / 2; step > 0; step >>= 1)
                        if (roff[wave][r + step] <= idx) r += step;
                    tab[wave][r * kStride + j] = __uint_as_float((uint32_t)(v[u] >> 32));
                    break;
                }
                at = nxt[j];
            }
        }
    }
    __syncthreads();

    const int64_t row = base + lane;
    if (lane >= ROWS || row >= ntotal) return;
    float acc = 0.0f;
    bool hit = false;
    if (lane < nrow) {
        const float* tr = tab[wave] + lane * kStride;
        for (int j = 0; j < m; ++j) {
            const float d = tr[j];
            if (d != 0.0f) {
                acc = acc + qw[j] * d;
                hit = true;
            }
        }
    }
    col[row] = hit ? acc : miss;
}

// The vector mover of css_index_remove_rows, one wave per source row r < nlist: a kept row's entries move to
// noff[map[r]] of the new buffer (map[r] = the row's new number, kLexNoRow when it goes).
__global__ __launch_bounds__(256) void k_sparse_move(const unsigned long long* __restrict__ ent, const int64_t* __restrict__ off,
                                                     const uint32_t* __restrict__ map, const int64_t* __restrict__ noff,
                                                     int64_t nlist, unsigned long long* __restrict__ nent) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= nlist) return;
    const uint32_t nr = map[r];
    if (nr == kLexNoRow) return;
    const int64_t s = off[r], cnt = off[r + 1] - s, d = noff[nr];
    for (int64_t i = lane; i < cnt; i += 64) nent[d + i] = ent[s + i];
}

// The k best rows of col[0, n) that are not -inf and whose mask bit is set (mask null: every row), larger first, ties
// to the lower row: block b's list (slice b of the column) into Dl / Il [k] (global ids; -1 and -inf in empty slots).
__device__ __forceinline__ void sparse_topk_block(const float* __restrict__ col, int64_t n, int64_t slice,
                                                  const uint32_t* __restrict__ mask, int k, int64_t id_base,
                                                  float* __restrict__ Dl, int64_t* __restrict__ Il) {
    __shared__ float ls[kWaves][CSS_KERNEL_MAX_K];
    __shared__ uint32_t li[kWaves][CSS_KERNEL_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = lane; i < k; i += 64) {
        ls[wave][i] = -INFINITY;
        li[wave][i] = kInvalidRow;
    }
    const int64_t begin = (int64_t)blockIdx.x * slice, end = std::min(begin + slice, n);
    for (int64_t c0 = begin + (int64_t)wave * 64; c0 < end; c0 += 64 * kWaves) {
        const int64_t row = c0 + lane;
        float s = -INFINITY;
        if (row < end) {
            s = col[row];
            if (mask != nullptr && !((mask[row >> 5] >> (row & 31)) & 1u)) s = -INFINITY;
        }
        // non-strict: an equal value with a lower row must still reach the comparator
        unsigned long long pass = __ballot(s != -INFINITY && s >= ls[wave][k - 1]);
        while (pass) {
            const int l = __ffsll((long long)pass) - 1;
            pass &= pass - 1;
            wave_insert<uint32_t>(ls[wave], li[wave], k, __shfl(s, l), (uint32_t)(c0 + l), lane);
        }
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < kWaves; ++w)
        for (int i = 0; i < k; ++i) {
            const uint32_t id = li[w][i];
            if (id == kInvalidRow) break;   // (wave uniform; a list is best first, its empty slots last)
            wave_insert<uint32_t>(ls[0], li[0], k, ls[w][i], id, lane);
        }
    for (int i = lane; i < k; i += 64) {
        const uint32_t id = li[0][i];
        Dl[i] = ls[0][i];
        Il[i] = id == kInvalidRow ? (int64_t)-1 : id_base + (int64_t)id;
    }
}
// block b's list into Dp / Ip [b][k]
__global__ __launch_bounds__(256) void k_sparse_topk(const float* __restrict__ col, int64_t n, int64_t slice,
                                                     const uint32_t* __restrict__ mask, int k, int64_t id_base,
                                                     float* __restrict__ Dp, int64_t* __restrict__ Ip) {
    sparse_topk_block(col, n, slice, mask, k, id_base, Dp + (size_t)blockIdx.x * k, Ip + (size_t)blockIdx.x * k);
}
// The same over the gridDim.y columns col[y][n] of a group of queries: block (b, y)'s list into Dp / Ip [b][y][k], the
// part layout of merge_parts with nq = gridDim.y.
__global__ __launch_bounds__(256) void k_sparse_topk_cols(const float* __restrict__ col, int64_t n, int64_t slice,
                                                          const uint32_t* __restrict__ mask, int k, int64_t id_base,
                                                          float* __restrict__ Dp, int64_t* __restrict__ Ip) {
    const size_t o = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * k;
    sparse_topk_block(col + (size_t)blockIdx.y * (size_t)n, n, slice, mask, k, id_base, Dp + o, Ip + o);
}

// D / I of css_index_search_sparse where nothing can hit: every slot padded
__global__ void k_sparse_pad(float* __restrict__ D, int64_t* __restrict__ I, int k) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    D[t] = -FLT_MAX;
    I[t] = -1;
}
