// css_where.h -- attribute filters on the flat index: a conjunction of comparisons over the per-row attribute columns
// (css_index_set_attr) turned into the allow bitmap every search variant takes.  Included by css_index.hip (inside its
// anonymous namespace, behind css_sparse.h).
//
// Columns.  An attribute column is a RowColumn: one dword per row, int32 or float32, coalesced for a wave that takes 64
// consecutive rows.  A clause is (column, op, operand); the row passes when every clause holds and its allow bit, where
// the call has a bitmap, is set.
//
// One comparison for both types.  The host turns the operand, and the kernel every loaded dword, into an unsigned KEY
// whose integer order is the order of the type: int32 v -> v ^ 0x80000000; float32 bits b -> -0.0 first folded onto
// +0.0, then ~b for negative and b | 0x80000000 for non-negative values.  Float keys are ordered like the floats from
// -inf to +inf with the denormals in their places, whatever the denormal mode of the build, and -0.0 == 0.0.  A stored
// NaN is recognised by its bits and fails every op but NE; a NaN OPERAND never reaches the kernel as a comparison: the
// host rewrites the clause to kWhereNever (NE: kWhereAlways).  These are the comparisons numpy makes on int32 and
// float32 arrays.
//
// IN / NOT_IN (int32 columns).  The operand is a bit table over [0, table_bits) at word `toff` of the call's table
// words; a value that is negative or >= table_bits is "not in".  LDS = true: all tables of the call, at most
// kWhereLdsWords words together, are copied into LDS once per block (a few codes: projects, chunk types, flags); the
// LDS is dynamic and sized by the call's table words, so a 2-word table does not cost the occupancy of a 32 KiB one.
// LDS = false: the lookups go to global memory, where a table of session codes (2^20 bits = 128 KiB) stays in L2.
//
// k_where.  A block of 4 waves takes tiles of kWhereTileRows = 1024 rows in a grid-stride loop (so the LDS copy of the
// tables is paid once per block, not once per tile); a wave takes kWhereGroups = 4 consecutive 64-row groups of the tile
// and two clauses per step, and keeps their 8 loads in flight together, one dword per lane, group and clause.  __ballot gives the 64 bits of a
// group; lanes 0..7 of the wave then store its 8 result words with ordinary stores, each only when the word lies below
// ceil(ntotal / 32) -- the second word of the last group can lie past the end.  Rows >= ntotal load nothing and have
// bit 0, so the tail of the last word is zero.  The set bits are counted from the ballots (wave-uniform), summed over
// the block's waves in LDS and added to the call's counter with ONE integer atomic per block: the order of integer
// additions does not matter, the count is the same every time.
// Traffic: 4 bytes per clause and row read, 1 bit per row read (allow) and written.
#pragma once

constexpr int kWhereTileRows = 1024;    // rows of one tile: 4 waves x kWhereGroups x 64 (tests/where_cases.py names it)
constexpr int kWhereGroups = 4;         // 64-row groups per wave and tile
constexpr int kWhereLdsWords = 8192;    // table words of a call that still go to LDS (32 KiB)
constexpr int kWhereNever = 8, kWhereAlways = 9;   // a clause with a NaN operand, decided on the host

static_assert(kWhereTileRows == 4 * kWhereGroups * 64, "a tile is what 4 waves take in one step");

// a clause as the kernel reads it (kernel arguments: scalar loads, no buffer to upload)
struct WhereArgs {
    const uint32_t* col[CSS_MAX_CLAUSES];
    uint32_t key[CSS_MAX_CLAUSES];     // the operand's key
    uint32_t toff[CSS_MAX_CLAUSES];    // IN / NOT_IN: first word of the table ...
    uint32_t tbits[CSS_MAX_CLAUSES];   // ... and its bits
    uint32_t kind[CSS_MAX_CLAUSES];    // op | (1 << 8 for a float32 column)
    int n;
};

__host__ __device__ __forceinline__ uint32_t where_key_i32(uint32_t v) { return v ^ 0x80000000u; }
__host__ __device__ __forceinline__ uint32_t where_key_f32(uint32_t b) {
    if ((b << 1) == 0u) b = 0u;   // -0.0 == 0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ bool where_is_nan(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u; }

// one clause as the kernel's registers hold it, and its answer for one loaded dword
struct WhereClause {
    const uint32_t* col;
    uint32_t key, toff, tbits;
    int op;
    bool f32;
};
__device__ __forceinline__ WhereClause where_clause(const WhereArgs& a, int c) {
    return WhereClause{a.col[c], a.key[c], a.toff[c], a.tbits[c], (int)(a.kind[c] & 0xFFu), (a.kind[c] >> 8) != 0u};
}
template <bool LDS>
__device__ __forceinline__ bool where_holds(const WhereClause& cl, uint32_t v, const uint32_t* tab,
                                            const uint32_t* __restrict__ tables) {
    if (cl.op == CSS_WHERE_IN || cl.op == CSS_WHERE_NOT_IN) {
        bool in = false;
        if (v < cl.tbits) {   // (unsigned: a negative value is above every table, tbits <= 2^27)
            const uint32_t w = cl.toff + (v >> 5);
            in = ((LDS ? tab[w] : tables[w]) >> (v & 31u)) & 1u;
        }
        return (cl.op == CSS_WHERE_IN) == in;
    }
    if (cl.op >= kWhereNever) return cl.op == kWhereAlways;
    if (cl.f32 && where_is_nan(v)) return cl.op == CSS_WHERE_NE;
    const uint32_t k = cl.f32 ? where_key_f32(v) : where_key_i32(v);
    switch (cl.op) {
    case CSS_WHERE_EQ: return k == cl.key;
    case CSS_WHERE_NE: return k != cl.key;
    case CSS_WHERE_LT: return k < cl.key;
    case CSS_WHERE_LE: return k <= cl.key;
    case CSS_WHERE_GT: return k > cl.key;
    default: return k >= cl.key;
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_where(const WhereArgs a, const uint32_t* __restrict__ tables, int table_words,
                                               const uint32_t* __restrict__ allow, int64_t ntotal, int64_t tiles,
                                               uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    extern __shared__ uint32_t tab[];   // LDS: table_words words (the launch sizes it), so a small table costs no occupancy
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LDS) {
        for (int i = tid; i < table_words; i += 256) tab[i] = tables[i];
        __syncthreads();
    }
    const int64_t nwords = (ntotal + 31) >> 5;
    uint32_t cnt = 0;   // wave-uniform
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kWhereTileRows + (int64_t)wave * (kWhereGroups * 64);
        bool p[kWhereGroups];
#pragma unroll
        for (int g = 0; g < kWhereGroups; ++g) {
            const int64_t r = base + g * 64 + lane;
            p[g] = r < ntotal;
            if (allow != nullptr && p[g]) p[g] = (allow[r >> 5] >> (r & 31)) & 1u;
        }
        // two clauses per step: the 2 * kWhereGroups loads are issued before the first value is looked at
        for (int c = 0; c < a.n; c += 2) {
            const bool two = c + 1 < a.n;
            const WhereClause c0 = where_clause(a, c), c1 = where_clause(a, two ? c + 1 : c);
            uint32_t v0[kWhereGroups], v1[kWhereGroups];
#pragma unroll
            for (int g = 0; g < kWhereGroups; ++g) {
                const int64_t r = base + g * 64 + lane;
                v0[g] = r < ntotal ? c0.col[r] : 0u;
            }
#pragma unroll
            for (int g = 0; g < kWhereGroups; ++g) {
                const int64_t r = base + g * 64 + lane;
                v1[g] = (two && r < ntotal) ? c1.col[r] : 0u;
            }
#pragma unroll
            for (int g = 0; g < kWhereGroups; ++g) p[g] = p[g] && where_holds<LDS>(c0, v0[g], tab, tables);
            if (two) {
#pragma unroll
                for (int g = 0; g < kWhereGroups; ++g) p[g] = p[g] && where_holds<LDS>(c1, v1[g], tab, tables);
            }
        }
        unsigned long long b[kWhereGroups];
#pragma unroll
        for (int g = 0; g < kWhereGroups; ++g) {
            b[g] = __ballot(p[g]);
            cnt += (uint32_t)__popcll(b[g]);
        }
        // the 2 * kWhereGroups words of the wave, one per lane
        if (lane < 2 * kWhereGroups) {
            unsigned long long bb = b[0];
#pragma unroll
            for (int g = 1; g < kWhereGroups; ++g)
                if ((lane >> 1) == g) bb = b[g];
            const int64_t w = (base >> 5) + lane;
            if (w < nwords) bits[w] = (uint32_t)(bb >> (32 * (lane & 1)));
        }
    }
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long s = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (s != 0ull) atomicAdd(count, s);
    }
}
