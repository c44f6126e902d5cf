// css_tokens_lists.h -- the MaxSim of MANY query matrices, each over a row list of its own, in one launch
// (css_index_maxsim_rows_batch; the re-rank stage of css_index_search_rerank_maxsim), and the two small kernels that
// stand around it in the two-stage search.  Included by css_index.hip behind css_tokens.h: the turn's head and tail,
// the query's fragments, the staged tile (TokTile) and the tile step are that header's, shared with k_tok_scores.
//
// k_tok_scores_l<P, MT, NB>.  Query b (tokens [qoff[b], qoff[b + 1]) of q) owns the list rows[b][0 .. f): row numbers,
// kTokNoRow = no row.  col[b][j] = the MaxSim of query b with row rows[b][j]; -inf for a miss (no row, a row >= T, an
// empty row).  A persistent grid of four-wave blocks as in k_tok_scores, but the query belongs to the TURN and not to
// the block: a turn is `per` <= 16 consecutive positions of ONE query's list (tq = ceil(f / per) turns per query, the
// last one partial: f need not be a multiple of per), and the nq tq turns of the call are dealt out in CONTIGUOUS
// chunks, wave after wave, so that a wave's consecutive turns stay within a query except at its chunk's query
// boundaries.  The wave keeps the A fragments of its turn's query in registers and reloads them only when the query
// changes (at f = 64 and per = 16 a wave with 8 turns reloads at most twice).  MT is that of the call's LONGEST query;
// a shorter query's tiles are zero-filled (tok_query_frags) and its tail adds its own mq maxima only, as in
// k_tok_scores_b.  Within a turn the tile sequence, the three stages in flight (fetch of tile i + 2, centroid gather
// of tile i + 1, decode and multiply of tile i) and the parks are k_tok_scores'; the step is tok_tile_step, so every
// element sees that kernel's MFMAs in that order on the same operand values, and col[b][j] has the bits of
// k_tok_scores for (q_b, [row]), raw and compressed.  No atomics and no cross-wave traffic: neither the grid, `per`,
// nq nor the position in the list changes the bits.
//
// Bounds.  A position is read only below f of its own query (tok_turn_head: pos < n = f), a row number only enters the
// offsets below s.nlist (kTokNoRow = 0xFFFFFFFF is never below it: the host refuses stores of 2^32 - 1 rows and more),
// a token index stays inside [beg, beg + md) (TokTile::fetch clamps), and col is written at the positions read.
#pragma once

constexpr uint32_t kTokNoRow = 0xFFFFFFFFu;

template <int P, int MT, int NB>
__global__ __launch_bounds__(64 * kWaves) void k_tok_scores_l(const TokStore s, const uint32_t* __restrict__ rows /* [nq][f] */,
                                                              int nq, int f, const unsigned short* __restrict__ q,
                                                              const int64_t* __restrict__ qoff /* [nq + 1] */, int per,
                                                              float* __restrict__ col /* [nq][f] */) {
    constexpr int KS = P / 32;
    typedef TokTile<P, NB> Tile;
    __shared__ float park[kWaves][kTokTurn * kTokPark];
    __shared__ float wl[16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lr = lane & 15, g = lane >> 4;
    const TokWeights w = tok_weights_stage<NB>(s.wts, wl);
    float* mypark = park[wave];
    const int64_t tq = (f + per - 1) / per, nturns = tq * nq;   // (1 <= per <= kTokTurn)
    // the wave's chunk of consecutive turns
    const int64_t nwaves = (int64_t)gridDim.x * kWaves, chunk = (nturns + nwaves - 1) / nwaves;
    const int64_t t0 = ((int64_t)blockIdx.x * kWaves + wave) * chunk, t1 = min(t0 + chunk, nturns);
    v8bf qa[MT][KS];
    int cur = -1, mq = 0;   // the query whose fragments the wave holds
    for (int64_t turn = t0; turn < t1; ++turn) {
        const int b = (int)(turn / tq);
        if (b != cur) {
            const int64_t qb = qoff[b];
            mq = __builtin_amdgcn_readfirstlane((int)(qoff[b + 1] - qb));
            tok_query_frags<P, MT>(q + (size_t)qb * P, mq, lr, g, qa);
            cur = b;
        }
        const uint32_t* list = rows + (size_t)b * f;
        int md_lane;
        int64_t beg_lane, pos;
        TokAt ld = tok_turn_head(s, list, f, nullptr, per, turn - b * tq, lane, md_lane, beg_lane, pos);   // the next tile to load ...
        TokAt at = ld;                                                                                     // ... and to multiply
        Tile b0, b1, b2;
        b0.code = b1.code = b2.code = 0u;   // (a buffer without a tile gathers centroid 0 and is never multiplied)
        auto load = [&](Tile& t) {
            if (ld.j >= kTokTurn) return;
            t.fetch(s, ld, lr, g);
            tok_next_tile(ld, md_lane, beg_lane);
        };
        v4f run[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) run[mt] = v4f{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        // tile i sits in buffer i % 3; its step fetches tile i + 2 and gathers the centroids of tile i + 1
        auto step = [&](Tile& c, Tile& nxt, Tile& nn) {
            load(nn);
            nxt.gather(s, g);
            tok_tile_step<MT>(qa, c, w, at, md_lane, beg_lane, run, mypark, lr, g);
        };
        load(b0);
        load(b1);
        b0.gather(s, g);
        while (true) {
            if (at.j >= kTokTurn) break;
            step(b0, b1, b2);
            if (at.j >= kTokTurn) break;
            step(b1, b2, b0);
            if (at.j >= kTokTurn) break;
            step(b2, b0, b1);
        }
        tok_turn_tail(mypark, lane, md_lane, mq, lane < per && pos < f, col + (size_t)b * f, pos);
    }
}

// The pool lists of a search (ids I [total] global, -1 = padding; their dense scores S) as row lists: id - id_base, and
// kTokNoRow for padding and for an entry with S < floor (a NaN floor compares false: no floor).
__global__ void k_rr_lists(const int64_t* __restrict__ I, const float* __restrict__ S, int64_t total, int64_t id_base,
                           float floor, uint32_t* __restrict__ rows) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t id = I[t];
    rows[t] = (id < 0 || S[t] < floor) ? kTokNoRow : (uint32_t)(id - id_base);
}

// The answer of the two-stage search from the ranked POSITIONS (Pp [nq][k], -1 = no entry; Dp their MaxSim) and the
// pool lists [nq][f]: D = the MaxSim, I = the pool's id, S = the pool's dense score, R = the position; an empty slot is
// padded as css_index_search_maxsim pads (D = S = -FLT_MAX, I = R = -1).
__global__ void k_rr_out(const float* __restrict__ Dp, const int64_t* __restrict__ Pp, const float* __restrict__ poolS,
                         const int64_t* __restrict__ poolI, int f, int k, int64_t total, float* __restrict__ D,
                         int64_t* __restrict__ I, float* __restrict__ S, int32_t* __restrict__ R) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t p = Pp[t];
    if (p < 0) {
        D[t] = -FLT_MAX;
        I[t] = -1;
        S[t] = -FLT_MAX;
        R[t] = -1;
        return;
    }
    const size_t e = (size_t)(t / k) * f + (size_t)p;
    D[t] = Dp[t];
    I[t] = poolI[e];
    S[t] = poolS[e];
    R[t] = (int32_t)p;
}
// every slot padded: an index without matrices
__global__ void k_rr_pad(int64_t total, float* __restrict__ D, int64_t* __restrict__ I, float* __restrict__ S,
                         int32_t* __restrict__ R) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    D[t] = -FLT_MAX;
    I[t] = -1;
    S[t] = -FLT_MAX;
    R[t] = -1;
}
