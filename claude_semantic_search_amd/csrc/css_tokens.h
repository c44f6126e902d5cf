// css_tokens.h -- token matrices on the flat index (late interaction, ColBERT): one [m, P] bf16 matrix per row in HBM,
// raw or as residual codes, and the MaxSim column of ONE query matrix over all rows, or over a list of rows.  Included
// by css_index.hip (inside its anonymous namespace, behind css_sparse.h and css_token_codec.h: it reuses kWaves,
// dpp_f32, v8bf, v4f, tok_v8s and the codec's decode; the column is ranked by k_sparse_topk_cols and the part merge).
// The pieces that make up the score -- the head and the tail of a turn, the query's fragments, the staged tile and the
// tile step -- are defined HERE and used by k_tok_scores, k_tok_scores_b (css_tokens_batch.h) and k_tok_ci
// (css_token_prune.h): the score is defined by instruction order.  ONE exception, for measured speed: k_tok_scores'
// step lambda carries the text of tok_tile_step and of TokTile::frag's decode; a change to either is made there too.
//
// Layout.  Row r < T (T = the leading rows that were given a matrix) owns tokens [off[r], off[r + 1]) of the store, so a
// row's matrix is ONE contiguous span: 2 P m bytes of `tok` in a raw store; 2 m bytes of `codes` and RB m of `res` in a
// compressed one (css_token_codec.h), with the centroid table `cent` and the 16 bucket weights `wts` beside them.
// Rows >= T have none; an empty row is a row without tokens.  The tokens that ColBERT's keep flags drop are not
// stored, so there are no flags here.
//
// The score (include/css_hip.h has the definition) is that of css_encoder_maxsim with every token kept, bit for bit:
// tok_tile_step keeps k_maxsim's operand roles and lane-to-k mapping (css_encoder_kernels.h).  A = query tokens (rows),
// B = doc tokens (columns): lane l holds the 16 bytes at k = 32 step + 8 (l >> 4) of query row 16 mt + (l & 15) and of
// doc token 16 tile + (l & 15), and C/D of doc column l & 15 for the query rows 16 mt + 4 (l >> 4) + i; the K steps go
// in ascending order into one accumulator per (mt, tile).  A C element depends on its own A row and B column alone, so
// every element sees the same instruction sequence on the same values as in k_maxsim; the maximum is order-free and the
// sum over the query's tokens has one order.  On a compressed store the B fragment is the DECODED token, formed in
// registers: the same MFMAs in the same order on the same operand values as over the decoded matrices.
//
// k_tok_scores<P, MT, NB> (MT = the query's tiles of 16 tokens; NB = 0: a raw store, NB = 1, 2, 4: the bits of a
// bucket).  A persistent grid of four-wave blocks.  The query is staged ONCE per block, straight into registers: a
// lane's A fragments are MT * P / 32 * 16 bytes (64 VGPRs at MT = 4, P = 128) and are read by every MFMA of the
// kernel, which an LDS copy would re-read at one ds_read_b128 per MFMA.
// Block b takes the runs of 4 * per consecutive rows b, b + grid, ...; wave w of the block takes the `per` <= 16 rows
// per * w .. per * w + per - 1 of the run (its "turn"): lanes 0 .. per - 1 read the rows' offsets and allow bits, a
// masked, empty or matrix-less row is dropped from the turn's live set before any of its tokens is loaded, and the
// wave walks the 16-token tiles of the live docs as ONE sequence -- tiles never span docs; the last tile of a doc
// re-reads the doc's last token in the lanes beyond its end and enters -inf for them.  `per` is 16 for a scan (few
// turns per wave would leave the prefetch nothing to run ahead into) and smaller where the rows are few, so that a
// re-rank of 64 rows runs on 64 waves and not on 4.
// Three stages are in flight, across doc boundaries, through three register buffers used in turn (no copies between
// them, so a wait is for one tile's loads only): tile i + 2 is fetched (non-temporal loads straight to VGPRs: every
// byte is used once by one wave -- 16 bytes per K step of a raw token, or the code and NB bytes of buckets per K
// step), the centroid fragments of tile i + 1 are gathered by its codes (ordinary loads through the caches: the table
// is C x 2 P bytes and every wave re-reads it; nothing to do on a raw store), tile i is decoded and multiplied.  At
// the end of a doc the running maxima are reduced over the 16 lanes of a row group with DPP (row16_allmax) and PARKED
// in the wave's LDS rows [16][65]; at the end of the turn lane d < per adds doc d's maxima in ascending query token,
// so the chains of up to 64 dependent adds of 16 docs run side by side once per turn, not once per doc, and the wave
// stores `per` consecutive floats of the column.  No atomics and no cross-wave traffic: the bits do not depend on the
// grid.  Rows come from `rows` (a list of n row numbers: css_index_maxsim_rows) or are 0 .. n - 1 (rows == null).
// Traffic per stored token of an allowed row: 2 P bytes raw, 2 + P NB / 8 compressed; 16 bytes of offsets and 4 of
// column per row.
#pragma once

constexpr int kTokQ = 64;             // query tokens at most (CSS_MAX_QUERY_TOKENS)
constexpr int kTokTurn = 16;          // docs of one wave's turn
constexpr int kTokPark = kTokQ + 1;   // floats between two docs' parked maxima: odd, the adding lanes hit distinct banks

// The store as the kernels see it (filled by tok_store of css_index.hip): `tok` in a raw store, `codes`, `res`, `cent`
// and `wts` ([16]) in a compressed one, the others null; the first `nlist` rows have offsets.
struct TokStore {
    const unsigned short* __restrict__ tok;
    const unsigned short* __restrict__ codes;
    const unsigned char* __restrict__ res;
    const unsigned short* __restrict__ cent;
    const float* __restrict__ wts;
    const int64_t* __restrict__ off;
    int64_t nlist;
};

__device__ __forceinline__ float tok_row16_allmax(float v) {   // row16_allmax of css_encoder_kernels.h
    v = fmaxf(v, dpp_f32<0xB1>(v));
    v = fmaxf(v, dpp_f32<0x4E>(v));
    v = fmaxf(v, dpp_f32<0x141>(v));
    v = fmaxf(v, dpp_f32<0x140>(v));
    return v;
}

// A position in a turn's tile sequence (wave uniform): doc j of the turn (kTokTurn: past the end), its tile t, its md
// tokens from token `beg` on; `live` holds the bits of the live docs behind j.
struct TokAt {
    unsigned live;
    int j, t, md;
    int64_t beg;
};
// to the first tile of the next live doc; lane d < 16 holds doc d's length and first token
__device__ __forceinline__ void tok_next_doc(TokAt& at, int md_lane, int64_t beg_lane) {
    at.j = at.live ? __ffs(at.live) - 1 : kTokTurn;
    at.live &= at.live - 1u;
    at.t = 0;
    const int src = at.j & (kTokTurn - 1);
    at.md = __builtin_amdgcn_readlane(md_lane, src);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)beg_lane, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)beg_lane >> 32), src);
    at.beg = (int64_t)((unsigned long long)hi << 32 | lo);
}
__device__ __forceinline__ void tok_next_tile(TokAt& at, int md_lane, int64_t beg_lane) {
    if (++at.t * 16 >= at.md) tok_next_doc(at, md_lane, beg_lane);
}

// The head of turn `turn` of `per` <= kTokTurn rows: lane d < per takes position pos = per turn + d of the n (row
// rows[pos], or pos itself under rows == null) and reads its length md_lane and first token beg_lane; a position
// beyond n and a masked, empty or matrix-less row keep md_lane = 0 and are not live.  Returns the first live doc's
// first tile.
__device__ __forceinline__ TokAt tok_turn_head(const TokStore& s, const uint32_t* __restrict__ rows, int64_t n,
                                               const uint32_t* __restrict__ mask, int per, int64_t turn, int lane,
                                               int& md_lane, int64_t& beg_lane, int64_t& pos) {
    pos = turn * per + (lane & 15);
    md_lane = 0;
    beg_lane = 0;
    if (lane < per && pos < n) {
        const int64_t row = rows != nullptr ? (int64_t)rows[pos] : pos;
        if (row < s.nlist && (mask == nullptr || ((mask[row >> 5] >> (row & 31)) & 1u))) {
            beg_lane = s.off[row];
            md_lane = (int)(s.off[row + 1] - beg_lane);
        }
    }
    TokAt at;
    at.live = (unsigned)__ballot(lane < per && md_lane > 0);
    tok_next_doc(at, md_lane, beg_lane);
    return at;
}

// The tail of a turn: a lane that owns a position (`mine`) adds its doc's parked maxima in ascending query token and
// stores col[pos]; -inf for a row that was not live.  (One wave writes and reads its own park rows: the LDS keeps a
// wave's accesses in order.)
__device__ __forceinline__ void tok_turn_tail(const float* mypark, int lane, int md_lane, int mq, bool mine,
                                              float* __restrict__ col, int64_t pos) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (mine) {
        float s = -__builtin_inff();
        if (md_lane > 0) {
            s = 0.f;
            const float* mx = mypark + lane * kTokPark;
            for (int i = 0; i < mq; ++i) s += mx[i];
        }
        col[pos] = s;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The query's A fragments: rows beyond mq inside its last tile are zeros, their results are never read
template <int P, int MT>
__device__ __forceinline__ void tok_query_frags(const unsigned short* __restrict__ q, int mq, int lr, int g,
                                                v8bf (&qa)[MT][P / 32]) {
    static_assert(P % 32 == 0 && P >= 32 && P <= 128, "whole K steps of the MFMA");
    static_assert(MT >= 1 && MT * 16 <= kTokQ, "the query's tiles");
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < P / 32; ++ks) {
            const int r = 16 * mt + lr;
            const uint4 v = r < mq ? *reinterpret_cast<const uint4*>(q + (size_t)r * P + 32 * ks + 8 * g) : make_uint4(0u, 0u, 0u, 0u);
            qa[mt][ks] = __builtin_bit_cast(v8bf, v);
        }
}

// A lane's share of one staged tile of 16 doc tokens, in three stages: fetch (what the store holds of token
// min(16 t + lr, md - 1) of the doc), gather (the centroid's fragments by the code; nothing on a raw store) and
// frag(ks), the bf16 B fragment of K step ks (decoded on a compressed store, a bit cast on a raw one).  A TokTile<P, 0>
// also carries fragments that were staged elsewhere (k_tok_scores_b reads them back from its ring).
template <int P, int NB>
struct TokTile {
    static constexpr int KS = P / 32, RB = P * NB / 8;
    unsigned code;    // (NB != 0) the centroid: a tile that was never fetched must hold a valid one to be gathered
    unsigned r[KS];   // (NB != 0) the packed buckets, NB bytes per K step
    tok_v8s f[KS];    // the raw fragments, or the gathered centroid's

    __device__ __forceinline__ void fetch(const TokStore& s, const TokAt& at, int lr, int g) {
        const size_t t = (size_t)at.beg + (size_t)min(at.t * 16 + lr, at.md - 1);
        if constexpr (NB == 0) {
            const unsigned short* drow = s.tok + t * P + 8 * g;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) f[ks] = __builtin_nontemporal_load(reinterpret_cast<const tok_v8s*>(drow + 32 * ks));
        } else {
            code = __builtin_nontemporal_load(s.codes + t);
            const unsigned char* rp = s.res + t * RB + NB * g;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) r[ks] = tok_res_load<NB>(rp + 4 * NB * ks);
        }
    }
    __device__ __forceinline__ void gather(const TokStore& s, int g) {
        if constexpr (NB != 0) {
            const unsigned short* crow = s.cent + (size_t)code * P + 8 * g;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) f[ks] = *reinterpret_cast<const tok_v8s*>(crow + 32 * ks);
        }
    }
    // (into a reference: returned by value, the fragment is coerced to integers on the way and the decode is then
    // packed two components to an instruction, at up to 19 more VGPRs)
    __device__ __forceinline__ void frag(int ks, const TokWeights& w, v8bf& d) const {
        if constexpr (NB == 0) {
            d = __builtin_bit_cast(v8bf, f[ks]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = tok_decode1(f[ks][j], tok_weight<NB>((r[ks] >> (NB * j)) & ((1u << NB) - 1u), w));
        }
    }
};

// One tile of the sequence against the query: the MFMAs (K steps outer and ascending, one fresh accumulator per mt) on
// the fragments of `cur`, -inf for the lanes beyond the doc's end, the running maxima, `at` to the next tile; behind a
// doc's last tile its maxima are reduced, parked for the adds of tok_turn_tail and reset.  No barrier.  Used by
// k_tok_scores_b; k_tok_scores carries this text in its step lambda (see there).
template <int MT, class Tile>
__device__ __forceinline__ void tok_tile_step(const v8bf (&qa)[MT][Tile::KS], const Tile& cur, const TokWeights& w, TokAt& at, int md_lane,
                                     int64_t beg_lane, v4f (&run)[MT], float* mypark, int lr, int g) {
    constexpr int KS = Tile::KS;
    const float ninf = -__builtin_inff();
    v4f acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        v8bf b;
        cur.frag(ks, w, b);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[mt][ks], b, acc[mt], 0, 0, 0);
    }
    const bool ok = at.t * 16 + lr < at.md;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) run[mt][i] = fmaxf(run[mt][i], ok ? acc[mt][i] : ninf);
    const int doc = at.j;
    tok_next_tile(at, md_lane, beg_lane);
    if (at.j == doc) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float m = tok_row16_allmax(run[mt][i]);
            if (lr == 0) mypark[doc * kTokPark + mt * 16 + 4 * g + i] = m;
            run[mt][i] = ninf;
        }
}

template <int P, int MT, int NB>
__global__ __launch_bounds__(64 * kWaves) void k_tok_scores(const TokStore s, const uint32_t* __restrict__ rows, int64_t n,
                                                            const uint32_t* __restrict__ mask,
                                                            const unsigned short* __restrict__ q, int mq, int per,
                                                            float* __restrict__ col) {
    constexpr int KS = P / 32;
    typedef TokTile<P, NB> Tile;
    __shared__ float park[kWaves][kTokTurn * kTokPark];
    __shared__ float wl[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const TokWeights w = tok_weights_stage<NB>(s.wts, wl);
    v8bf qa[MT][KS];
    tok_query_frags<P, MT>(q, mq, lr, g, qa);
    float* mypark = park[wave];
    const int64_t nturns = (n + per - 1) / per;   // (1 <= per <= kTokTurn)
    for (int64_t turn = (int64_t)blockIdx.x * kWaves + wave; turn < nturns; turn += (int64_t)gridDim.x * kWaves) {
        int md_lane;
        int64_t beg_lane, pos;
        TokAt ld = tok_turn_head(s, rows, n, mask, per, turn, lane, md_lane, beg_lane, pos);   // the next tile to load ...
        TokAt at = ld;                                                                         // ... and the next to multiply
        Tile b0, b1, b2;
        b0.code = b1.code = b2.code = 0u;   // (a buffer without a tile gathers centroid 0 and is never multiplied)
        auto load = [&](Tile& b) {
            if (ld.j >= kTokTurn) return;
            b.fetch(s, ld, lr, g);
            tok_next_tile(ld, md_lane, beg_lane);
        };
        v4f run[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) run[mt] = v4f{-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        // tile i sits in buffer i % 3; its step fetches tile i + 2 and gathers the centroids of tile i + 1
        auto step = [&](Tile& cur, Tile& nxt, Tile& nn) {
            load(nn);
            nxt.gather(s, g);
            // tok_tile_step's text with the decode of TokTile::frag in it, and not a call of either: written here, the
            // compiler schedules the NB = 1 and 4 kernels as it did before the merge; through the functions the scan at
            // P = 96, NB = 4 measured 4.5 % slower with the same registers.  k_tok_scores_b uses the functions.
            const float ninf = -__builtin_inff();
            v4f acc[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                v8bf b;
                if constexpr (NB == 0) {
                    b = __builtin_bit_cast(v8bf, cur.f[ks]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) b[j] = tok_decode1(cur.f[ks][j], tok_weight<NB>((cur.r[ks] >> (NB * j)) & ((1u << NB) - 1u), w));
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[mt][ks], b, acc[mt], 0, 0, 0);
            }
            const bool ok = at.t * 16 + lr < at.md;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) run[mt][i] = fmaxf(run[mt][i], ok ? acc[mt][i] : ninf);
            const int doc = at.j;
            tok_next_tile(at, md_lane, beg_lane);
            if (at.j == doc) return;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float m = tok_row16_allmax(run[mt][i]);
                    if (lr == 0) mypark[doc * kTokPark + mt * 16 + 4 * g + i] = m;
                    run[mt][i] = ninf;
                }
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
        tok_turn_tail(mypark, lane, md_lane, mq, lane < per && pos < n, col, pos);
    }
}
