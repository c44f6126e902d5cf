// css_lexical.h -- the lexical side of css_index_search_hybrid: per-row term lists in HBM and the BM25 column of ONE
// query over all rows.  Included by css_index.hip (inside its anonymous namespace).
//
// Layout.  Row r < T (T = the leading rows that were given a list) owns entries [off[r], off[r + 1]) of `ent`: one
// uint32 per distinct term, term << 8 | min(tf, 255), ascending by term, and dl[r] = the tokens the row was given,
// repeats included.  Rows >= T have no list.  df[2^24] counts the rows that hold a term, *total is the sum of dl; both
// are kept current with integer atomics (one add per entry that comes or goes), so they do not depend on arrival order.
//
// k_lex_scores.  A wave owns the entry span of 64 consecutive rows and streams it with one dword per lane and four
// loads in flight, whatever the row lengths are.  An entry is looked up in a 4096-slot LDS byte table of the query terms
// (term & 4095 -> 1 + the first query term with these low bits, 0: none; query terms that share their low bits are
// chained through nxt[]), so an entry that matches nothing costs one LDS byte and a match one compare -- 32 compares
// per entry made the pass issue-bound at 32 terms (DESIGN.md 3.2j has both measurements).  A match (row, j) writes its
// tf byte into the wave's LDS table [64 rows][32 terms]; the row of an entry comes from a binary search in the wave's
// 65 offsets in LDS.  Terms are
// distinct within a row and within the query, so no two lanes write one byte.  Lane r then forms the sum of row r in
// QUERY-TERM order -- not in the order the entries lie in memory -- in fp32 with the operations of the header comment
// (include/css_hip.h), and the wave stores one coalesced segment of the column.  The table rows are 9 dwords apart
// (36 bytes), so the 64 lanes read distinct LDS banks.  Traffic: 4 E + 12 N bytes read, 4 N written.
#pragma once

constexpr int kLexTabWords = 9;        // dwords per table row: 32 tf bytes + one dword of padding
constexpr uint32_t kLexNoRow = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_lex_scores(const uint32_t* __restrict__ ent, const int64_t* __restrict__ off,
                                                    const uint32_t* __restrict__ dl, int64_t nlist, int64_t ntotal,
                                                    const uint32_t* __restrict__ qterms, const float* __restrict__ qweights,
                                                    int m, float k1, float c0, float c1, float* __restrict__ lex) {
    __shared__ uint32_t slot_w[1024];   // 4096 byte slots
    __shared__ unsigned char nxt[CSS_MAX_QUERY_TERMS];
    __shared__ uint32_t qt[CSS_MAX_QUERY_TERMS];
    __shared__ float qw[CSS_MAX_QUERY_TERMS];
    __shared__ uint32_t roff[kWaves][65];
    __shared__ uint32_t tab[kWaves][64 * kLexTabWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* slot = reinterpret_cast<unsigned char*>(slot_w);
    for (int i = tid; i < 1024; i += 256) slot_w[i] = 0u;
    if (tid < CSS_MAX_QUERY_TERMS) {
        qt[tid] = tid < m ? qterms[tid] : 0u;
        qw[tid] = tid < m ? qweights[tid] : 0.f;
    }
    for (int i = lane; i < 64 * kLexTabWords; i += 64) tab[wave][i] = 0u;
    const int64_t base = ((int64_t)blockIdx.x * kWaves + wave) * 64;
    const int nrow = (int)std::min<int64_t>(std::max<int64_t>(nlist - base, 0), 64);   // rows of this wave with a list
    int64_t s = 0;
    uint32_t mine = 0u, last = 0u, dlr = 0u;
    if (nrow > 0) {
        s = off[base];
        mine = (uint32_t)(off[base + std::min(lane, nrow)] - s);   // (a wave's span is below 64 * 2^20 entries)
        last = (uint32_t)(off[base + nrow] - s);
        if (lane < nrow) dlr = dl[base + lane];
    }
    roff[wave][lane] = mine;
    if (lane == 0) roff[wave][64] = last;
    __syncthreads();
    if (tid == 0)   // chains in ascending j: built from the back, each term put in front of its slot
        for (int j = m - 1; j >= 0; --j) {
            const uint32_t hslot = qt[j] & 4095u;
            nxt[j] = slot[hslot];
            slot[hslot] = (unsigned char)(j + 1);
        }
    __syncthreads();

    const uint32_t span = last;
    const uint32_t* e = ent + s;
    unsigned char* tb = reinterpret_cast<unsigned char*>(tab[wave]);
    for (uint32_t i0 = 0; i0 < span; i0 += 256) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t idx = i0 + u * 64 + lane;
            v[u] = idx < span ? __builtin_nontemporal_load(e + idx) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t idx = i0 + u * 64 + lane;
            const uint32_t term = v[u] >> 8;
            uint32_t at = idx < span ? slot[term & 4095u] : 0u;
            while (at != 0u) {
                const int j = (int)at - 1;
                if (qt[j] == term) {
                    int r = 0;   // the last row whose first entry is at or below idx
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1)
                        if (roff[wave][r + step] <= idx) r += step;
                    tb[r * (kLexTabWords * 4) + j] = (unsigned char)(v[u] & 255u);
                    break;
                }
                at = nxt[j];
            }
        }
    }
    __syncthreads();

    const int64_t row = base + lane;
    if (row >= ntotal) return;
    float acc = 0.0f;
    if (lane < nrow) {
        const float K = c0 + c1 * (float)dlr;
        const float k1p = k1 + 1.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const uint32_t word = tab[wave][lane * kLexTabWords + w];
            if (word == 0u) continue;
#pragma unroll
            for (int bt = 0; bt < 4; ++bt) {
                const uint32_t tf = (word >> (8 * bt)) & 255u;
                if (tf > 0u) {
                    const float ft = (float)tf;
                    const float g = (ft * k1p) / (ft + K);
                    acc = acc + qw[w * 4 + bt] * g;
                }
            }
        }
    }
    lex[row] = acc;
}

// df[term] += delta for every entry of ent[0, count): the lists that come (delta = 1) or go (delta = -1, as a wrapping add)
__global__ __launch_bounds__(256) void k_lex_df_add(const uint32_t* __restrict__ ent, int64_t count, uint32_t* __restrict__ df,
                                                    uint32_t delta) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) atomicAdd(&df[ent[i] >> 8], delta);
}

// *total += (or -=) the sum of dl[0, n): one 64-bit add per wave
__global__ __launch_bounds__(256) void k_lex_len_add(const uint32_t* __restrict__ dl, int64_t n, unsigned long long* __restrict__ total,
                                                     int negate) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned long long sum = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) sum += dl[i];
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum != 0ull) atomicAdd(total, negate ? 0ull - sum : sum);
}

// The list mover of css_index_remove_rows, one wave per source row r < nlist.  map[r] = the row's new number, or
// kLexNoRow when it goes: a kept row's entries and dl move to noff[map[r]] of the new buffers, a removed row's entries
// leave df and its dl leaves *total.
__global__ __launch_bounds__(256) void k_lex_move(const uint32_t* __restrict__ ent, const int64_t* __restrict__ off,
                                                  const uint32_t* __restrict__ dl, const uint32_t* __restrict__ map,
                                                  const int64_t* __restrict__ noff, int64_t nlist, uint32_t* __restrict__ nent,
                                                  uint32_t* __restrict__ ndl, uint32_t* __restrict__ df,
                                                  unsigned long long* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= nlist) return;
    const int64_t s = off[r], cnt = off[r + 1] - s;
    const uint32_t nr = map[r];
    if (nr != kLexNoRow) {
        const int64_t d = noff[nr];
        for (int64_t i = lane; i < cnt; i += 64) nent[d + i] = ent[s + i];
        if (lane == 0) ndl[nr] = dl[r];
    } else {
        for (int64_t i = lane; i < cnt; i += 64) atomicAdd(&df[ent[s + i] >> 8], 0xFFFFFFFFu);
        if (lane == 0 && dl[r] != 0u) atomicAdd(total, 0ull - (unsigned long long)dl[r]);
    }
}

// css_index_term_stats: out[j] = df[terms[j]] for j < m, out[m] = *total
__global__ __launch_bounds__(256) void k_lex_stats(const uint32_t* __restrict__ terms, int m, const uint32_t* __restrict__ df,
                                                   const unsigned long long* __restrict__ total, long long* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) out[i] = (long long)df[terms[i]];
    if (i == m) out[m] = (long long)*total;
}

// L of css_index_search_hybrid: the column's value at the k returned rows (col null: no column was formed), 0 in padded slots
__global__ void k_lex_gather(const int64_t* __restrict__ I, int k, int64_t id_base, const float* __restrict__ col,
                             float* __restrict__ L) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const int64_t id = I[t];
    L[t] = (col && id >= 0) ? col[id - id_base] : 0.0f;
}
