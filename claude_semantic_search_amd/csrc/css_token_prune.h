// css_token_prune.h -- candidate generation for MaxSim on a compressed store (PLAID's centroid interaction): rank every
// row by the MaxSim of its tokens' CENTROIDS, which reads only the 2-byte code of a token and a small table, and leave
// the decode to the few thousand best.  Included by css_index.hip behind css_tokens.h (it reuses TokStore, TokAt,
// tok_next_doc, tok_turn_head / tok_turn_tail, tok_query_frags, kTokTurn, kTokPark, v8bf, v4f, kWaves).
// include/css_hip.h has the definitions in bits.
//
// k_tok_ctable<P>.  S[c, s] = dot(q_s, centroid_c) into tab [C][W], W = 16 MT floats per centroid, formed as
// k_tok_scores forms the dot of query token s with a doc token equal to centroid c: query tokens as rows of A, the 16
// centroids of a tile as columns of B, the K steps of 32 ascending into one accumulator per (mt, tile), so S[c, s] has
// the bits of that kernel's C element.  One wave per tile of 16 centroids; centroids beyond C are not written; the
// query rows beyond mq inside the last tile are zeros (never summed).
//
// k_tok_ci<WP>.  A[r] = sum over s ascending of max over the row's tokens t of S[code_t, s]: by construction the score
// that k_tok_scores gives the matrix centroids[codes of r], bit for bit (the maximum is order-free, the sum is the same
// ascending chain over the same parked maxima).  The grid, the turns, and the off / mask / T handling in front of any
// load are those of k_tok_scores.  A wave walks the live docs of its turn in chunks of 64 tokens: lane l loads the code
// of token l of the chunk (non-temporal: used once; the chunk after it is in flight meanwhile), then WP lanes read the
// table row of one token, lane s its S[code, s]: one coalesced read of 4 W bytes through the caches, 64 / WP tokens per
// instruction (WP = 16, 32, 64 for a query of up to 16, 32, 64 tokens), 8 instructions in flight.  The running maximum
// per s is folded over the lane groups at the end of the doc and parked in the wave's LDS rows, and lane d adds doc d's
// maxima at the end of the turn as k_tok_scores does.  No atomics, no cross-wave traffic: the bits do not depend on the
// grid.
//
// The select.  The first ncand rows of lexsort((row, -A)) among the rows that are no miss (-inf), as a list in
// ASCENDING ROW ORDER, exact, for any n: keys are the order-preserving uint32 image of the float (-0.0 as +0.0);
// four histogram passes of 8 bits each over the rows that match the prefix found so far (k_sel_hist: LDS histogram,
// integer atomics, order-free), every block re-deriving the prefix from the histograms of the passes before it (sel_resolve);
// then the threshold key with the number `need` of rows EQUAL to it that still belong; per-block counts of rows above
// and equal over slices of kSelSlice rows (k_sel_count); and the ordered write (k_sel_write): a block sums the counts
// of the blocks before it, and a row above the threshold lands at (rows above before it) + min(rows equal before it,
// need), a row equal to it likewise while its rank among the equal ones is below need.  Fewer than ncand rows that are
// no miss: all of them.
#pragma once

constexpr int kSelSlice = 4096;     // rows of one block of the compaction
constexpr int kSelMaxBlocks = 1024;   // blocks of a histogram pass at most (grid stride)
// words of the select's state in front of the per-block counts: 4 x 256 bins | threshold key, need, all, count out
constexpr int kSelHist = 4 * 256, kSelState = kSelHist + 4;

template <int P>
__global__ __launch_bounds__(64 * kWaves) void k_tok_ctable(const unsigned short* __restrict__ cent, int C,
                                                            const unsigned short* __restrict__ q, int mq, int MT,
                                                            float* __restrict__ tab) {
    constexpr int KS = P / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const int c0 = (blockIdx.x * kWaves + wave) * 16;
    if (c0 >= C) return;   // (wave uniform; no barrier below)
    const int cc = min(c0 + lr, C - 1), W = 16 * MT;
    v8bf b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        b[ks] = __builtin_bit_cast(v8bf, *reinterpret_cast<const uint4*>(cent + (size_t)cc * P + 32 * ks + 8 * g));
    for (int mt = 0; mt < MT; ++mt) {
        v8bf a[1][KS];   // the query's tile mt
        tok_query_frags<P, 1>(q + (size_t)16 * mt * P, mq - 16 * mt, lr, g, a);
        v4f acc = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][ks], b[ks], acc, 0, 0, 0);
        // C/D: centroid column lr, the query rows 16 mt + 4 g + i
        if (c0 + lr < C) *reinterpret_cast<v4f*>(tab + (size_t)(c0 + lr) * W + 16 * mt + 4 * g) = acc;
    }
}

template <int WP>
__global__ __launch_bounds__(64 * kWaves) void k_tok_ci(const TokStore store, const float* __restrict__ tab, int W,
                                                        const uint32_t* __restrict__ rows, int64_t n,
                                                        const uint32_t* __restrict__ mask, int mq, int per,
                                                        float* __restrict__ col) {
    static_assert(WP == 16 || WP == 32 || WP == 64, "lanes of one token's table row");
    constexpr int TPI = 64 / WP, U = 8;   // tokens per instruction, instructions in flight
    __shared__ float park[kWaves][kTokTurn * kTokPark];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & (WP - 1), sub = lane / WP;
    const float ninf = -__builtin_inff();
    const float* trow = tab + min(s, W - 1);   // (W = 48 under WP = 64: the lanes beyond W re-read column W - 1)
    float* mypark = park[wave];
    const int64_t nturns = (n + per - 1) / per;   // (1 <= per <= kTokTurn)
    for (int64_t turn = (int64_t)blockIdx.x * kWaves + wave; turn < nturns; turn += (int64_t)gridDim.x * kWaves) {
        int md_lane;
        int64_t beg_lane, pos;
        // the next chunk of 64 tokens to load (t counts chunks here) ...
        TokAt ld = tok_turn_head(store, rows, n, mask, per, turn, lane, md_lane, beg_lane, pos);
        TokAt at = ld;   // ... and the next to look up
        auto load = [&]() -> unsigned {
            if (ld.j >= kTokTurn) return 0u;
            const unsigned c = __builtin_nontemporal_load(store.codes + (size_t)ld.beg + (size_t)min(ld.t * 64 + lane, ld.md - 1));
            if (++ld.t * 64 >= ld.md) tok_next_doc(ld, md_lane, beg_lane);
            return c;
        };
        unsigned cnext = load();
        float run = ninf;
        while (at.j < kTokTurn) {
            const unsigned ccur = cnext;
            cnext = load();
            const int cnt = min(64, at.md - at.t * 64);   // tokens of this chunk
            for (int t0 = 0; t0 < cnt; t0 += TPI * U) {
                float v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {   // (a lane beyond the chunk repeats its last token: the maximum does not move)
                    const int src = min(t0 + u * TPI + sub, cnt - 1);
                    unsigned c;
                    if constexpr (WP == 64) c = (unsigned)__builtin_amdgcn_readlane((int)ccur, src);
                    else c = (unsigned)__shfl((int)ccur, src, 64);
                    v[u] = trow[(size_t)c * W];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) run = fmaxf(run, v[u]);
            }
            const int doc = at.j;
            if (++at.t * 64 >= at.md) tok_next_doc(at, md_lane, beg_lane);
            if (at.j == doc) continue;
            // the doc's last chunk: the lane groups are folded and the maxima parked for the adds at the end of the turn
            if constexpr (WP <= 32) run = fmaxf(run, __shfl_xor(run, 32, 64));
            if constexpr (WP <= 16) run = fmaxf(run, __shfl_xor(run, 16, 64));
            if (lane < WP && s < W) mypark[doc * kTokPark + s] = run;
            run = ninf;
        }
        tok_turn_tail(mypark, lane, md_lane, mq, lane < per && pos < n, col, pos);
    }
}

// ------------------------------------------------------------------ the select
// larger float <=> larger key; -0.0 and +0.0 share a key; -inf (a miss) has the lowest key of all and is never counted
__device__ __forceinline__ uint32_t sel_key(float v) {
    const uint32_t u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// What the histograms of passes 0 .. npass - 1 say: the key's leading 8 npass bits in `prefix`, and how many of the
// rows that share them are still to take (`need`, from ncand); all = fewer than ncand rows are no miss (every one is
// taken; only pass 0 can tell).  A block of 256 threads; sh = 258 words of LDS; every thread returns the same values.
__device__ __forceinline__ void sel_resolve(const uint32_t* __restrict__ hist, int npass, uint32_t ncand, uint32_t* sh,
                                            uint32_t& prefix, uint32_t& need, bool& all) {
    const int d = threadIdx.x;
    prefix = 0u;
    need = ncand;
    all = false;
    for (int p = 0; p < npass && !all; ++p) {
        const uint32_t h = hist[p * 256 + d];
        __syncthreads();   // (the words of the pass before are read)
        sh[d] = h;
        if (d == 0) sh[256] = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t incl = h;   // rows of the bins d .. 255
        for (int o = 1; o < 256; o <<= 1) {
            const uint32_t t = d + o < 256 ? sh[d + o] : 0u;
            __syncthreads();
            incl += t;
            sh[d] = incl;
            __syncthreads();
        }
        const uint32_t above = incl - h;
        if (above < need && incl >= need) {   // (one bin at most)
            sh[256] = (uint32_t)d;
            sh[257] = above;
        }
        __syncthreads();
        const uint32_t bin = sh[256];
        if (bin == 0xFFFFFFFFu) {
            all = true;
        } else {
            prefix = prefix << 8 | bin;
            need -= sh[257];
        }
    }
    __syncthreads();
}

// pass `pass` (0 .. 3): the histogram of the next 8 key bits over the rows that are no miss and match the prefix
__global__ __launch_bounds__(256) void k_sel_hist(const float* __restrict__ col, int64_t n, uint32_t ncand, int pass,
                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t sh[258];
    __shared__ uint32_t lh[256];
    uint32_t prefix, need;
    bool all;
    sel_resolve(hist, pass, ncand, sh, prefix, need, all);
    if (all) return;   // (block uniform)
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = col[i];
        if (v == -__builtin_inff()) continue;
        const uint32_t key = sel_key(v);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&lh[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(&hist[pass * 256 + threadIdx.x], c);
}

// block b: the rows above the threshold and the rows equal to it in its slice, into cnt[2 b], cnt[2 b + 1]; block 0
// also leaves [threshold key, need, all] in st
__global__ __launch_bounds__(256) void k_sel_count(const float* __restrict__ col, int64_t n, uint32_t ncand,
                                                   const uint32_t* __restrict__ hist, uint32_t* __restrict__ st,
                                                   uint32_t* __restrict__ cnt) {
    __shared__ uint32_t sh[258];
    __shared__ uint32_t red[2][kWaves];
    uint32_t thr, need;
    bool all;
    sel_resolve(hist, 4, ncand, sh, thr, need, all);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[0] = thr;
        st[1] = need;
        st[2] = all ? 1u : 0u;
    }
    const int64_t begin = (int64_t)blockIdx.x * kSelSlice, end = min(begin + (int64_t)kSelSlice, n);
    uint32_t gt = 0u, eq = 0u;
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
        const float v = col[i];
        if (v == -__builtin_inff()) continue;
        const uint32_t key = sel_key(v);
        gt += (all || key > thr) ? 1u : 0u;
        eq += (!all && key == thr) ? 1u : 0u;
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
        gt += __shfl_xor(gt, x, 64);
        eq += __shfl_xor(eq, x, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = gt;
        red[1][threadIdx.x >> 6] = eq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[2 * blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        cnt[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// The ordered write: block b's taken rows behind those of the blocks before it, in row order, into cand (row numbers)
// and approx (their values); block 0 leaves the number of rows taken in st[3].  The slots behind it are not written.
__global__ __launch_bounds__(256) void k_sel_write(const float* __restrict__ col, int64_t n, const uint32_t* __restrict__ cnt,
                                                   int nblk, uint32_t ncand, uint32_t* __restrict__ st,
                                                   uint32_t* __restrict__ cand, float* __restrict__ approx) {
    __shared__ unsigned long long red[kWaves];
    __shared__ uint32_t wg[kWaves], we[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t thr = st[0], need = st[1];
    const bool all = st[2] != 0u;
    // the rows above and equal in the blocks before this one (block 0: in every block, for the count)
    const int upto = blockIdx.x == 0 ? nblk : (int)blockIdx.x;
    unsigned long long g = 0ull, e = 0ull;
    for (int b = tid; b < upto; b += 256) {
        g += cnt[2 * b];
        e += cnt[2 * b + 1];
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) {
        g += __shfl_xor(g, x, 64);
        e += __shfl_xor(e, x, 64);
    }
    if (lane == 0) red[wave] = g;
    __syncthreads();
    g = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    if (lane == 0) red[wave] = e;
    __syncthreads();
    e = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    uint32_t gbef = (uint32_t)g, ebef = (uint32_t)e;
    if (blockIdx.x == 0) {
        if (tid == 0) st[3] = (uint32_t)(g + (e < need ? e : (unsigned long long)need));
        gbef = 0u;
        ebef = 0u;
    }
    const int64_t begin = (int64_t)blockIdx.x * kSelSlice, end = min(begin + (int64_t)kSelSlice, n);
    for (int64_t c0 = begin; c0 < end; c0 += 256) {
        const int64_t i = c0 + tid;
        float v = -__builtin_inff();
        if (i < end) v = col[i];
        const bool live = v != -__builtin_inff();
        const uint32_t key = sel_key(v);
        const bool isg = live && (all || key > thr), ise = live && !all && key == thr;
        const unsigned long long bg = __ballot(isg), be = __ballot(ise);
        if (lane == 0) {
            wg[wave] = (uint32_t)__popcll(bg);
            we[wave] = (uint32_t)__popcll(be);
        }
        __syncthreads();
        uint32_t g0 = gbef, e0 = ebef, gall = gbef, eall = ebef;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) {
                g0 += wg[w];
                e0 += we[w];
            }
            gall += wg[w];
            eall += we[w];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        g0 += (uint32_t)__popcll(bg & below);
        e0 += (uint32_t)__popcll(be & below);
        if (isg || (ise && e0 < need)) {
            const uint32_t at = g0 + min(e0, need);
            if (at < ncand) {   // (always: the counts add up to at most ncand)
                cand[at] = (uint32_t)i;
                approx[at] = v;
            }
        }
        gbef = gall;
        ebef = eall;
        __syncthreads();
    }
}

// The candidates as the results of css_index_maxsim_candidates: global ids and approximate scores of the nc slots (-1
// behind the count), and the count in the id slot behind them
__global__ __launch_bounds__(256) void k_tok_cand_out(const uint32_t* __restrict__ cand, const float* __restrict__ approx,
                                                      const uint32_t* __restrict__ st, int64_t nc, int64_t id_base,
                                                      float* __restrict__ D, int64_t* __restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > nc) return;
    const uint32_t cn = st[3];
    if (i == nc) {
        I[i] = (int64_t)cn;
        D[i] = 0.f;
    } else {
        I[i] = i < (int64_t)cn ? id_base + (int64_t)cand[i] : (int64_t)-1;
        D[i] = i < (int64_t)cn ? approx[i] : 0.f;
    }
}

// The positions in the candidate list that the top-k of css_index_search_maxsim_pruned returns become global ids; the
// candidate count goes into the id slot behind them
__global__ __launch_bounds__(256) void k_tok_cand_ids(const uint32_t* __restrict__ cand, const uint32_t* __restrict__ st,
                                                      int k, int64_t id_base, float* __restrict__ D, int64_t* __restrict__ I) {
    const int i = threadIdx.x;
    if (i < k) {
        const int64_t p = I[i];
        if (p >= 0) I[i] = id_base + (int64_t)cand[p];
    } else if (i == k) {
        I[i] = (int64_t)st[3];
        D[i] = 0.f;
    }
}
