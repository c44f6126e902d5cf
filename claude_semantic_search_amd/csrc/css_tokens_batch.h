// css_tokens_batch.h -- the MaxSim columns of a GROUP of query matrices in one pass over the token store
// (css_index_search_maxsim_batch).  Included by css_index.hip behind css_token_codec.h (it reuses TokAt, tok_next_doc /
// tok_next_tile, tok_row16_allmax, kTokTurn, kTokPark, tok_v8s, tok_res_load, tok_weight, tok_decode1, v8bf, v4f).
//
// k_tok_scores_b<P, MT, NB, G>.  A persistent grid of blocks of G waves; wave w owns query slot w of the group and
// keeps that query's A fragments in registers exactly as k_tok_scores does (MT = the tiles of the group's LONGEST
// query; a shorter query's tiles are zero-filled and its sums stop at its own length).  NB = 0: the raw store;
// NB = 1, 2, 4: the compressed store.  The BLOCK takes the turns of 16 consecutive rows b, b + grid, ...: every wave
// reads the same 16 offsets and allow bits and so derives the same live set and the same tile sequence as
// k_tok_scores' wave would for that turn.  The sequence is cut into rounds of G tiles.  Wave w STAGES tile G r + w of
// round r: it performs k_tok_scores' per-lane load (k_tok_scores_c's load, gather and decode on a compressed store)
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
__global__ __launch_bounds__(64 * G) void k_tok_scores_b(const unsigned short* __restrict__ tok,
                                                         const unsigned short* __restrict__ codes,
                                                         const unsigned char* __restrict__ res,
                                                         const unsigned short* __restrict__ cent,
                                                         const float* __restrict__ wts /* [16] */,
                                                         const int64_t* __restrict__ off, int64_t nlist, int64_t n,
                                                         const uint32_t* __restrict__ mask,
                                                         const unsigned short* __restrict__ q /* the batch's tokens */,
                                                         const int64_t* __restrict__ qoff /* [nslots + 1] */, int nslots,
                                                         float* __restrict__ col /* [G][n] */) {
    static_assert(P % 32 == 0 && P >= 32 && P <= 128, "whole K steps of the MFMA");
    static_assert(MT >= 1 && MT * 16 <= kTokQ, "the group's longest query in tiles");
    static_assert(NB == 0 || NB == 1 || NB == 2 || NB == 4, "bits of a bucket (0: the raw store)");
    static_assert(G >= 2 && G <= 16, "waves of a block");
    constexpr int KS = P / 32, RB = P * NB / 8;
    __shared__ float park[G][kTokTurn * kTokPark];
    __shared__ uint4 ring[2][G][KS * 64];
    __shared__ float wl[16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lr = lane & 15, g = lane >> 4;
    const float ninf = -__builtin_inff();
    float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
    if constexpr (NB != 0) {
        if constexpr (NB == 4) {
            if (threadIdx.x < 16) wl[threadIdx.x] = wts[threadIdx.x];
            __syncthreads();
        }
        w0 = wts[0], w1 = wts[1], w2 = wts[2], w3 = wts[3];
    }
    // the slot's query, once; an empty slot (mq = 0, wave uniform) multiplies nothing and stores nothing
    int mq = 0;
    const unsigned short* qw = q;
    if (wave < nslots) {
        const int64_t qb = qoff[wave];
        mq = __builtin_amdgcn_readfirstlane((int)(qoff[wave + 1] - qb));
        qw = q + (size_t)qb * P;
    }
    v8bf qa[MT][KS];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int r = 16 * mt + lr;
            const uint4 v = r < mq ? *reinterpret_cast<const uint4*>(qw + (size_t)r * P + 32 * ks + 8 * g) : make_uint4(0u, 0u, 0u, 0u);
            qa[mt][ks] = __builtin_bit_cast(v8bf, v);
        }
    float* mypark = park[wave];
    float* mycol = col + (size_t)wave * (size_t)n;
    struct SBuf {   // a staged tile: raw fragments, or codes + buckets + gathered centroid fragments
        bool has;
        unsigned code;
        unsigned r[KS];
        tok_v8s f[KS];
    };
    const int64_t nturns = (n + kTokTurn - 1) / kTokTurn;
    for (int64_t turn = blockIdx.x; turn < nturns; turn += gridDim.x) {
        const int64_t pos = turn * kTokTurn + lr;
        int md_lane = 0;
        int64_t beg_lane = 0;
        if (lane < kTokTurn && pos < n) {
            if (pos < nlist && (mask == nullptr || ((mask[pos >> 5] >> (pos & 31)) & 1u))) {
                beg_lane = off[pos];
                md_lane = (int)(off[pos + 1] - beg_lane);
            }
        }
        TokAt ld;   // the first tile of the next round to stage ...
        ld.live = (unsigned)__ballot(lane < kTokTurn && md_lane > 0);
        tok_next_doc(ld, md_lane, beg_lane);
        TokAt at = ld;   // ... and the next tile to multiply
        // the wave's tile of the round at `ld` (the w-th of it), `ld` to the round behind
        auto pick = [&](TokAt& mine) {
            mine.j = kTokTurn;
            for (int i = 0; i < G; ++i) {
                if (ld.j >= kTokTurn) break;
                if (i == wave) mine = ld;
                tok_next_tile(ld, md_lane, beg_lane);
            }
        };
        // k_tok_scores' load (NB = 0) or k_tok_scores_c's load of codes and buckets
        auto fetch = [&](SBuf& s) {
            TokAt mine;
            pick(mine);
            s.has = mine.j < kTokTurn;
            if (!s.has) return;
            const size_t t = (size_t)mine.beg + (size_t)min(mine.t * 16 + lr, mine.md - 1);
            if constexpr (NB == 0) {
                const unsigned short* drow = tok + t * P + 8 * g;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s.f[ks] = __builtin_nontemporal_load(reinterpret_cast<const tok_v8s*>(drow + 32 * ks));
            } else {
                s.code = __builtin_nontemporal_load(codes + t);
                const unsigned char* rp = res + t * RB + NB * g;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s.r[ks] = tok_res_load<(NB ? NB : 1)>(rp + 4 * NB * ks);
            }
        };
        auto gather = [&](SBuf& s) {
            if (!s.has) return;
            const unsigned short* crow = cent + (size_t)s.code * P + 8 * g;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s.f[ks] = *reinterpret_cast<const tok_v8s*>(crow + 32 * ks);
        };
        // the staged tile into the wave's place of ring half `h`, decoded first on a compressed store
        auto put = [&](SBuf& s, int h) {
            if (!s.has) return;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if constexpr (NB == 0) {
                    ring[h][wave][ks * 64 + lane] = __builtin_bit_cast(uint4, s.f[ks]);
                } else {
                    v8bf d;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        d[j] = tok_decode1(s.f[ks][j], tok_weight<(NB ? NB : 1)>((s.r[ks] >> (NB * j)) & ((1u << NB) - 1u), wl, w0, w1, w2, w3));
                    ring[h][wave][ks * 64 + lane] = __builtin_bit_cast(uint4, d);
                }
            }
        };
        v4f run[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) run[mt] = v4f{ninf, ninf, ninf, ninf};
        // the tiles of one round from ring half `h`, each as a step of k_tok_scores; tile i + 1 is read before tile i's MFMAs
        auto consume = [&](int h) {
            if (mq == 0) {   // an empty slot only walks the sequence: it leaves the LDS and the matrix core to the others
                for (int i = 0; i < G && at.j < kTokTurn; ++i) tok_next_tile(at, md_lane, beg_lane);
                return;
            }
            uint4 cur[KS], nxt[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) cur[ks] = ring[h][0][ks * 64 + lane];
#pragma unroll 2
            for (int i = 0; i < G; ++i) {
                if (at.j >= kTokTurn) break;
                if (i + 1 < G) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) nxt[ks] = ring[h][i + 1][ks * 64 + lane];
                }
                v4f acc[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[mt][ks], __builtin_bit_cast(v8bf, cur[ks]), acc[mt], 0, 0, 0);
                const bool ok = at.t * 16 + lr < at.md;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) run[mt][e] = fmaxf(run[mt][e], ok ? acc[mt][e] : ninf);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) cur[ks] = nxt[ks];
                const int doc = at.j;
                tok_next_tile(at, md_lane, beg_lane);
                if (at.j == doc) continue;
                // the doc's last tile: its maxima are parked for the adds at the end of the turn
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float m = tok_row16_allmax(run[mt][e]);
                        if (lr == 0) mypark[doc * kTokPark + mt * 16 + 4 * g + e] = m;
                        run[mt][e] = ninf;
                    }
            }
        };
        if constexpr (NB == 0) {
            SBuf s0;
            fetch(s0);
            for (int h = 0; at.j < kTokTurn; h ^= 1) {
                put(s0, h);
                __syncthreads();
                fetch(s0);
                consume(h);
            }
        } else {
            // three stages in flight: codes of round r + 2 loaded, centroids of round r + 1 gathered, round r decoded
            SBuf s0, s1;
            s0.code = s1.code = 0u;
            fetch(s0);
            fetch(s1);
            gather(s0);
            while (at.j < kTokTurn) {
                put(s0, 0);
                __syncthreads();
                gather(s1);
                fetch(s0);
                consume(0);
                if (at.j >= kTokTurn) break;
                put(s1, 1);
                __syncthreads();
                gather(s0);
                fetch(s1);
                consume(1);
            }
        }
        // (a wave writes and reads its own park rows: the LDS keeps a wave's accesses in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < kTokTurn && pos < n && wave < nslots) {
            float s = ninf;
            if (md_lane > 0) {
                s = 0.f;
                const float* mx = mypark + lane * kTokPark;
                for (int i = 0; i < mq; ++i) s += mx[i];
            }
            mycol[pos] = s;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __syncthreads();   // the next turn writes half 0 of the ring again
    }
}
