// css_tokens_batch.h -- the MaxSim columns of a GROUP of query matrices in one pass over the token store
// (css_index_search_maxsim_batch).  Included by css_index.hip behind css_tokens.h: the turn's head and tail, the
// query's fragments, the staged tile (TokTile) and the tile step are that header's, shared with k_tok_scores.
//
// k_tok_scores_b<P, MT, NB, G>.  A persistent grid of blocks of G waves; wave w owns query slot w of the group and
// keeps that query's A fragments in registers exactly as k_tok_scores does (MT = the tiles of the group's LONGEST
// query; a shorter query's tiles are zero-filled and its sums stop at its own length).  NB = 0: the raw store;
// NB = 1, 2, 4: the compressed store.  The BLOCK takes the turns of 16 consecutive rows b, b + grid, ...: every wave
// reads the same 16 offsets and allow bits and so derives the same live set and the same tile sequence as
// k_tok_scores' wave would for that turn.  The sequence is cut into rounds of G tiles.  Wave w STAGES tile G r + w of
// round r: it performs k_tok_scores' per-lane fetch (and its gather and decode on a compressed store)
// one round ahead into registers and writes the bf16 fragments to the ring in LDS in FRAGMENT ORDER -- the 16 bytes
// lane l feeds to K step ks at ((ks * 64) + l) * 16 -- so that every wave's ds_read_b128 of a tile is linear and
// conflict free.  After ONE block barrier per round all G waves multiply all G tiles of the round with their own
// query.  The ring holds two rounds: round r + 1 is written while stragglers still read round r, and the barrier of
// round r + 1 is what frees round r's half for round r + 2.  The stored token (or its code, buckets and centroid row)
// is therefore read once per GROUP and decoded once per group.
//
// The score keeps its one definition: element (query token s, doc token t) sees the same MFMAs in the same order on
// the same operand values as in k_tok_scores (the staging wave's registers hold exactly the bytes k_tok_scores' lane
// would hold; the LDS moves them unchanged), the per-doc maxima are reduced, parked ([16][65] floats per wave) and
// added per wave in ascending query token as there.  No atomics, no cross-block traffic: neither the group, the slot
// nor the grid changes the bits.
//
// Barriers.  Every __syncthreads sits on block-uniform control flow: the round loop runs while `at` (the same value in
// every wave) has a tile, a wave whose slot is empty (nq % G != 0) or whose staged tile does not exist takes part in
// every barrier and only skips its stores, and a turn without a live doc runs no round in any wave.  One more barrier
// ends a turn: the next turn's first round reuses half 0 of the ring.
#pragma once

template <int P, int MT, int NB, int G>
__global__ __launch_bounds__(64 * G) void k_tok_scores_b(const TokStore s, int64_t n, const uint32_t* __restrict__ mask,
                                                         const unsigned short* __restrict__ q /* the batch's tokens */,
                                                         const int64_t* __restrict__ qoff /* [nslots + 1] */, int nslots,
                                                         float* __restrict__ col /* [G][n] */) {
    static_assert(G >= 2 && G <= 16, "waves of a block");
    constexpr int KS = P / 32;
    typedef TokTile<P, NB> Tile;
    __shared__ float park[G][kTokTurn * kTokPark];
    __shared__ uint4 ring[2][G][KS * 64];
    __shared__ float wl[16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lr = lane & 15, g = lane >> 4;
    const TokWeights w = tok_weights_stage<NB>(s.wts, wl);
    // the slot's query, once; an empty slot (mq = 0, wave uniform) multiplies nothing and stores nothing
    int mq = 0;
    const unsigned short* qw = q;
    if (wave < nslots) {
        const int64_t qb = qoff[wave];
        mq = __builtin_amdgcn_readfirstlane((int)(qoff[wave + 1] - qb));
        qw = q + (size_t)qb * P;
    }
    v8bf qa[MT][KS];
    tok_query_frags<P, MT>(qw, mq, lr, g, qa);
    float* mypark = park[wave];
    float* mycol = col + (size_t)wave * (size_t)n;
    const int64_t nturns = (n + kTokTurn - 1) / kTokTurn;
    for (int64_t turn = blockIdx.x; turn < nturns; turn += gridDim.x) {
        int md_lane;
        int64_t beg_lane, pos;
        // the first tile of the next round to stage ...
        TokAt ld = tok_turn_head(s, nullptr, n, mask, kTokTurn, turn, lane, md_lane, beg_lane, pos);
        TokAt at = ld;   // ... and the next tile to multiply
        // the wave's tile of the round at `ld` (the w-th of it) is fetched, if there is one; `ld` to the round behind
        auto fetch = [&](Tile& t, bool& has) {
            TokAt mine;
            mine.j = kTokTurn;
            for (int i = 0; i < G; ++i) {
                if (ld.j >= kTokTurn) break;
                if (i == wave) mine = ld;
                tok_next_tile(ld, md_lane, beg_lane);
            }
            has = mine.j < kTokTurn;
            if (has) t.fetch(s, mine, lr, g);
        };
        // the staged tile into the wave's place of ring half `h`, decoded first on a compressed store
        auto put = [&](const Tile& t, bool has, int h) {
            if (!has) return;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                v8bf d;
                t.frag(ks, w, d);
                ring[h][wave][ks * 64 + lane] = __builtin_bit_cast(uint4, d);
            }
        };
        v4f run[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) run[mt] = v4f{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        // the tiles of one round from ring half `h`, each as a step of k_tok_scores; tile i + 1 is read before tile i's MFMAs
        auto consume = [&](int h) {
            if (mq == 0) {   // an empty slot only walks the sequence: it leaves the LDS and the matrix core to the others
                for (int i = 0; i < G && at.j < kTokTurn; ++i) tok_next_tile(at, md_lane, beg_lane);
                return;
            }
            TokTile<P, 0> cur, nxt;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) cur.f[ks] = __builtin_bit_cast(tok_v8s, ring[h][0][ks * 64 + lane]);
#pragma unroll 2
            for (int i = 0; i < G; ++i) {
                if (at.j >= kTokTurn) break;
                if (i + 1 < G) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) nxt.f[ks] = __builtin_bit_cast(tok_v8s, ring[h][i + 1][ks * 64 + lane]);
                }
                tok_tile_step<MT>(qa, cur, w, at, md_lane, beg_lane, run, mypark, lr, g);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) cur.f[ks] = nxt.f[ks];
            }
        };
        Tile s0, s1;
        bool has0, has1;
        if constexpr (NB == 0) {
            fetch(s0, has0);
            for (int h = 0; at.j < kTokTurn; h ^= 1) {
                put(s0, has0, h);
                __syncthreads();
                fetch(s0, has0);
                consume(h);
            }
        } else {
            // three stages in flight: codes of round r + 2 fetched, centroids of round r + 1 gathered, round r decoded
            fetch(s0, has0);
            fetch(s1, has1);
            if (has0) s0.gather(s, g);
            while (at.j < kTokTurn) {
                put(s0, has0, 0);
                __syncthreads();
                if (has1) s1.gather(s, g);
                fetch(s0, has0);
                consume(0);
                if (at.j >= kTokTurn) break;
                put(s1, has1, 1);
                __syncthreads();
                if (has0) s0.gather(s, g);
                fetch(s1, has1);
                consume(1);
            }
        }
        tok_turn_tail(mypark, lane, md_lane, mq, lane < kTokTurn && pos < n && wave < nslots, mycol, pos);
        __syncthreads();   // the next turn writes half 0 of the ring again
    }
}
