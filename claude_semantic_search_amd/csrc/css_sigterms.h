// css_sigterms.h -- significant terms: how many rows of a selection hold each term (css_index_subset_terms), and the
// terms that are over-represented in the selection against a background (css_index_significant_terms).  Included by
// css_index.hip (inside its anonymous namespace), behind css_lexical.h whose lists it reads.
//
// k_sig_count.  A scatter-count over the lists of css_lexical.h into a zeroed uint32 table [2^24]: +1 per entry of
// every selected row.  A wave owns 64 consecutive rows at a time, as in k_lex_scores, reads the two mask words of its
// rows and goes on to its next 64 rows at once when both are zero, so ten selected rows cost their own entries and
// 8 bytes of mask per 64 rows of the corpus.  A wave walks its selected rows as RUNS of consecutive set bits: a run's
// entries are one contiguous span, streamed with one dword per lane and four loads in flight, and no entry needs its
// row looked up (a full selection is one run per wave; the rows' offsets sit one per lane and are read by shuffle).
// Integer atomics only: the counts do not depend on arrival order.
//
// Frequent terms.  A term that most rows hold would send one global add per row to one address.  Each block keeps an
// LDS table of `slots` (term, count) pairs, hashed by term: an entry claims its slot (compare-and-swap on the tag) or
// finds its own term there and adds in LDS; an entry whose slot holds another term adds to the global table directly.
// The grid is ONE block of 16 waves per CU; a block strides over the 1024-row groups and flushes ONCE at its end, one
// global add per claimed slot.  A term in every row then costs one global add per block instead of one per row; a rare
// term costs an LDS pair and the same one global add.  (Four 4-wave blocks per CU flushed four times as many adds to the
// addresses of the frequent terms and took 10 % longer over every row, 2.7 times longer over 5 %: DESIGN.md 3.2l.)  Which terms get slots depends on arrival order, the sums do not.
// slots = 0: no table, every entry is a global add (css_index_set_sigterm_slots moves between the two; the integers
// are the same).
//
// k_sig_nz_* / k_sig_compact.  The non-zero slots of a table, ascending by term, with their counts: per-block counts
// (4096 slots a block), one scan of the 4096 block counts, an ordered write.
//
// k_sig_score and the select.  One pass over the 2^24 slots qualifies (fg >= min_count, fg * BG > bg * FG in uint64)
// and scores (JLH in float64, one rounding per operation) and appends (score bits, term) to a candidate list.  The key
// of the order -- score descending, then term ascending -- has 88 bits: the float64 bits of a positive score order as
// integers, and below them 0xFFFFFF - term.  The m-th best key is found exactly by a radix select, eleven byte passes
// over the candidates (histogram in LDS, then one small launch that picks the byte); the keys at or above it are
// gathered (they are distinct, so exactly min(m, candidates)) and one block sorts them.
#pragma once

constexpr uint32_t kSigEmpty = 0xFFFFFFFFu;   // a free LDS slot (terms are below 2^24); the term of an unused output
constexpr int kSigMaxSlots = 4096;            // 32 KB of LDS per block
constexpr int kSigWaves = 16;                 // waves per block of k_sig_count: one table serves 1024 rows at a time
constexpr int kSigSpan = 4096;                // table slots per block of the compaction
constexpr int kSigBlocks = (int)(CSS_TERM_SPACE / kSigSpan);
constexpr int kSigDigits = 11;                // bytes of the key: 8 of the score, 3 of 0xFFFFFF - term

struct SigState {
    uint32_t nc;          // candidates appended by k_sig_score
    uint32_t want;        // min(m, nc)
    uint32_t remaining;   // the rank still looked for among the keys that match the prefix
    uint32_t nout;        // cursor of k_sig_gather
    unsigned long long phi;   // prefix of the m-th key: score bits ...
    uint32_t plo;             // ... and 0xFFFFFF - term
    uint32_t total;           // non-zero slots (k_sig_nz_scan)
    uint32_t hist[256];
    uint32_t blockcnt[kSigBlocks], blockoff[kSigBlocks];
    unsigned long long sel_hi[CSS_MAX_SIG_TERMS];
    uint32_t sel_lo[CSS_MAX_SIG_TERMS];
};

__device__ __forceinline__ void sig_add(uint32_t term, uint32_t* tag, uint32_t* cnt, int slots, int shift,
                                        uint32_t* __restrict__ table) {
    if (slots) {
        const uint32_t slot = (term * 2654435761u) >> shift;
        const uint32_t prev = atomicCAS(&tag[slot], kSigEmpty, term);
        if (prev == kSigEmpty || prev == term) {
            atomicAdd(&cnt[slot], 1u);
            return;
        }
    }
    atomicAdd(&table[term], 1u);
}

// slots: 0 or a power of two in [16, kSigMaxSlots], shift = 32 - log2(slots); dynamic LDS: 2 * slots dwords
__global__ __launch_bounds__(64 * kSigWaves) void k_sig_count(const uint32_t* __restrict__ ent, const int64_t* __restrict__ off,
                                                   int64_t nlist, int64_t ntotal, const uint32_t* __restrict__ mask,
                                                   int slots, int shift, uint32_t* __restrict__ table) {
    extern __shared__ uint32_t sig_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* tag = sig_lds;
    uint32_t* cnt = sig_lds + slots;
    for (int i = tid; i < slots; i += 64 * kSigWaves) {
        tag[i] = kSigEmpty;
        cnt[i] = 0u;
    }
    __syncthreads();
    const int64_t groups = (nlist + 64 * kSigWaves - 1) / (64 * kSigWaves);
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t base = (g * kSigWaves + wave) * 64;
        const int nrow = (int)std::min<int64_t>(std::max<int64_t>(nlist - base, 0), 64);   // rows of this wave with a list
        uint32_t w0 = 0u, w1 = 0u;
        if (nrow > 0) {
            w0 = mask ? mask[base >> 5] : 0xFFFFFFFFu;
            w1 = mask ? (base + 32 < ntotal ? mask[(base >> 5) + 1] : 0u) : 0xFFFFFFFFu;
        }
        w0 = __builtin_amdgcn_readfirstlane(w0);
        w1 = __builtin_amdgcn_readfirstlane(w1);
        unsigned long long sel = (unsigned long long)w1 << 32 | w0;
        if (nrow < 64) sel &= (1ull << nrow) - 1ull;
        if (sel == 0ull) continue;   // none of the wave's 64 rows is selected: two mask words were read (no barrier below)
        const int64_t s = off[base];
        // lane r holds the offset of row r within the wave's span (lanes beyond the rows: its end)
        const uint32_t mine = (uint32_t)(off[base + std::min(lane, nrow)] - s);   // (a span is below 64 * 2^20 entries)
        const uint32_t last = (uint32_t)(off[base + nrow] - s);
        const uint32_t* e = ent + s;
        unsigned long long m = sel;
        while (m != 0ull) {   // (wave-uniform) one run of consecutive selected rows [r0, r0 + run) per turn
            const int r0 = __builtin_ctzll(m);
            const unsigned long long rest = ~(m >> r0);
            const int run = rest != 0ull ? __builtin_ctzll(rest) : 64 - r0;
            const uint32_t a = __shfl(mine, r0, 64), b = r0 + run < 64 ? __shfl(mine, r0 + run, 64) : last;
            for (uint32_t i0 = a; i0 < b; i0 += 256) {
                uint32_t v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t idx = i0 + u * 64 + lane;
                    v[u] = idx < b ? __builtin_nontemporal_load(e + idx) : 0u;
                }
                // a tag never changes once it is claimed: four plain LDS reads in flight settle the common case (the
                // term owns its slot already) with one LDS add; everything else takes the claiming path
                uint32_t slot[4], seen[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    slot[u] = slots ? ((v[u] >> 8) * 2654435761u) >> shift : 0u;
                    seen[u] = slots ? tag[slot[u]] : kSigEmpty;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (i0 + u * 64 + lane >= b) continue;
                    if (seen[u] == v[u] >> 8) atomicAdd(&cnt[slot[u]], 1u);
                    else sig_add(v[u] >> 8, tag, cnt, slots, shift, table);
                }
            }
            m = r0 + run >= 64 ? 0ull : m & ~((1ull << (r0 + run)) - 1ull);
        }
    }
    __syncthreads();
    for (int i = tid; i < slots; i += 64 * kSigWaves)
        if (tag[i] != kSigEmpty) atomicAdd(&table[tag[i]], cnt[i]);
}

// blockcnt[b] = the non-zero slots of table[b * kSigSpan, (b + 1) * kSigSpan)
__global__ __launch_bounds__(256) void k_sig_nz_count(const uint32_t* __restrict__ table, SigState* __restrict__ st) {
    __shared__ uint32_t wsum[kWaves];
    const int tid = threadIdx.x;
    const uint32_t* t = table + (size_t)blockIdx.x * kSigSpan;
    uint32_t c = 0u;
    for (int i = tid; i < kSigSpan; i += 256) c += t[i] != 0u;
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) st->blockcnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// blockoff = the exclusive scan of blockcnt, total = its sum.  One block.
__global__ __launch_bounds__(256) void k_sig_nz_scan(SigState* __restrict__ st) {
    constexpr int per = kSigBlocks / 256;
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x;
    uint32_t c = 0u;
    for (int i = 0; i < per; ++i) c += st->blockcnt[tid * per + i];
    part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0u;
        for (int i = 0; i < 256; ++i) {
            const uint32_t x = part[i];
            part[i] = run;
            run += x;
        }
        st->total = run;
    }
    __syncthreads();
    uint32_t run = part[tid];
    for (int i = 0; i < per; ++i) {
        st->blockoff[tid * per + i] = run;
        run += st->blockcnt[tid * per + i];
    }
}

// (term, count) of the non-zero slots, ascending by term, into the first `cap` places
__global__ __launch_bounds__(256) void k_sig_compact(const uint32_t* __restrict__ table, const SigState* __restrict__ st,
                                                     uint32_t cap, uint32_t* __restrict__ terms_out,
                                                     uint32_t* __restrict__ fg_out) {
    __shared__ uint32_t wsum[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t run = st->blockoff[blockIdx.x];
    for (int j = 0; j < kSigSpan; j += 256) {
        const uint32_t term = (uint32_t)blockIdx.x * kSigSpan + j + tid;
        const uint32_t v = table[term];
        const unsigned long long b = __ballot(v != 0u);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = run + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (v != 0u && pos < cap) {
            terms_out[pos] = term;
            fg_out[pos] = v;
        }
        run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// qualify, score, append.  FG, BG >= 1; bg >= fg wherever fg >= 1 (the selection lies within the background).
__global__ __launch_bounds__(256) void k_sig_score(const uint32_t* __restrict__ fg, const uint32_t* __restrict__ bg,
                                                   unsigned long long FG, unsigned long long BG, uint32_t min_count,
                                                   uint32_t cap, unsigned long long* __restrict__ key,
                                                   uint32_t* __restrict__ term_out, SigState* __restrict__ st) {
    const int lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * 256u;
    // (every lane of a wave makes the same number of turns: 2^24 is a multiple of the stride's wave part)
    for (uint32_t t0 = blockIdx.x * 256u + (threadIdx.x & ~63u); t0 < CSS_TERM_SPACE; t0 += stride) {
        const uint32_t t = t0 + lane;
        const uint32_t f = fg[t];
        bool ok = false;
        double sc = 0.0;
        if (f >= min_count) {
            const uint32_t b = bg[t];
            if ((unsigned long long)f * BG > (unsigned long long)b * FG) {
                const double p = (double)f / (double)FG;
                const double q = (double)b / (double)BG;
                sc = (p - q) * (p / q);
                ok = true;
            }
        }
        const unsigned long long bal = __ballot(ok);
        if (bal == 0ull) continue;
        uint32_t at = 0u;
        if (lane == 0) at = atomicAdd(&st->nc, (uint32_t)__popcll(bal));
        at = __shfl(at, 0, 64) + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (ok && at < cap) {
            key[at] = (unsigned long long)__double_as_longlong(sc);
            term_out[at] = t;
        }
    }
}

__device__ __forceinline__ uint32_t sig_digit(unsigned long long hi, uint32_t lo, int d) {
    return d < 8 ? (uint32_t)(hi >> (56 - 8 * d)) & 255u : (lo >> (16 - 8 * (d - 8))) & 255u;
}
// do the first d bytes of the key equal those of the prefix?
__device__ __forceinline__ bool sig_match(unsigned long long hi, uint32_t lo, unsigned long long phi, uint32_t plo, int d) {
    if (d == 0) return true;
    if (d <= 8) return ((hi ^ phi) >> (64 - 8 * d)) == 0ull;
    return hi == phi && ((lo ^ plo) >> (24 - 8 * (d - 8))) == 0u;
}

// hist[byte d of the key] over the candidates whose first d bytes match the prefix
__global__ __launch_bounds__(256) void k_sig_hist(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ term,
                                                  uint32_t cap, int d, SigState* __restrict__ st) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t n = std::min(st->nc, cap);
    const unsigned long long phi = st->phi;
    const uint32_t plo = st->plo;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned long long hi = key[i];
        const uint32_t lo = 0xFFFFFFu - term[i];
        if (sig_match(hi, lo, phi, plo, d)) atomicAdd(&h[sig_digit(hi, lo, d)], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x] != 0u) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// byte d of the m-th best key: the largest byte with at least `remaining` matching keys at or above it.  One wave;
// clears hist for the next pass.
__global__ __launch_bounds__(64) void k_sig_pick(int d, uint32_t m, uint32_t cap, SigState* __restrict__ st) {
    if (threadIdx.x == 0) {
        if (d == 0) {
            st->want = std::min(m, std::min(st->nc, cap));
            st->remaining = st->want;
        }
        uint32_t rem = st->remaining;
        if (rem > 0u) {
            uint32_t above = 0u;
            int bin = 255;
            for (; bin > 0; --bin) {
                const uint32_t c = st->hist[bin];
                if (above + c >= rem) break;
                above += c;
            }
            st->remaining = rem - above;
            if (d < 8) st->phi |= (unsigned long long)bin << (56 - 8 * d);
            else st->plo |= (uint32_t)bin << (16 - 8 * (d - 8));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256; i += 64) st->hist[i] = 0u;
}

// the keys at or above the m-th best: exactly `want` of them (keys are distinct)
__global__ __launch_bounds__(256) void k_sig_gather(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ term,
                                                    uint32_t cap, SigState* __restrict__ st) {
    const uint32_t n = std::min(st->nc, cap);
    if (st->want == 0u) return;
    const unsigned long long phi = st->phi;
    const uint32_t plo = st->plo;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned long long hi = key[i];
        const uint32_t lo = 0xFFFFFFu - term[i];
        if (hi > phi || (hi == phi && lo >= plo)) {
            const uint32_t at = atomicAdd(&st->nout, 1u);
            if (at < CSS_MAX_SIG_TERMS) {
                st->sel_hi[at] = hi;
                st->sel_lo[at] = lo;
            }
        }
    }
}

// One block of CSS_MAX_SIG_TERMS threads: the gathered keys sorted best first, and the m output slots written --
// out: [256 scores (float64 bits) | 256 terms | 256 fg | 256 bg | n_out] in 64-bit words
__global__ __launch_bounds__(CSS_MAX_SIG_TERMS) void k_sig_final(const uint32_t* __restrict__ fg, const uint32_t* __restrict__ bg,
                                                                 const SigState* __restrict__ st, unsigned long long* __restrict__ out) {
    constexpr int N = CSS_MAX_SIG_TERMS;
    __shared__ unsigned long long hi[N];
    __shared__ uint32_t lo[N];
    const int tid = threadIdx.x;
    const uint32_t n = st->want;
    hi[tid] = (uint32_t)tid < n ? st->sel_hi[tid] : 0ull;   // (a real score is positive: the fillers sort last)
    lo[tid] = (uint32_t)tid < n ? st->sel_lo[tid] : 0u;
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            const int o = tid ^ j;
            if (o > tid) {
                const bool lower = hi[tid] < hi[o] || (hi[tid] == hi[o] && lo[tid] < lo[o]);   // [tid] sorts after [o]
                if (lower == ((tid & k) == 0)) {
                    const unsigned long long th = hi[tid];
                    const uint32_t tl = lo[tid];
                    hi[tid] = hi[o];
                    lo[tid] = lo[o];
                    hi[o] = th;
                    lo[o] = tl;
                }
            }
        }
    __syncthreads();
    uint32_t* terms = reinterpret_cast<uint32_t*>(out + N);
    uint32_t* ofg = terms + N;
    uint32_t* obg = ofg + N;
    const bool real = (uint32_t)tid < n;
    const uint32_t term = real ? 0xFFFFFFu - lo[tid] : kSigEmpty;
    out[tid] = real ? hi[tid] : 0ull;
    terms[tid] = term;
    ofg[tid] = real ? fg[term] : 0u;
    obg[tid] = real ? bg[term] : 0u;
    if (tid == 0) out[N + 3 * N / 2] = n;
}
