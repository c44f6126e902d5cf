// css_tokens.h -- token matrices on the flat index (late interaction, ColBERT): one [m, P] bf16 matrix per row in HBM and
// the MaxSim column of ONE query matrix over all rows, or over a list of rows.  Included by css_index.hip (inside its
// anonymous namespace, behind css_sparse.h: it reuses kWaves, kLexNoRow, dpp_f32, v8bf and v4f; the column is ranked by
// k_sparse_topk and the part merge).
//
// Layout.  Row r < T (T = the leading rows that were given a matrix) owns tokens [off[r], off[r + 1]) of `tok`, P bf16
// each, so a row's matrix is ONE contiguous span of 2 P m bytes.  Rows >= T have none; an empty row is a row without
// tokens.  The tokens that ColBERT's keep flags drop are not stored, so there are no flags here.
//
// The score (include/css_hip.h has the definition) is that of css_encoder_maxsim with every token kept, bit for bit:
// k_tok_scores keeps k_maxsim's operand roles and lane-to-k mapping (css_encoder_kernels.h).  A = query tokens (rows),
// B = doc tokens (columns): lane l holds the 16 bytes at k = 32 step + 8 (l >> 4) of query row 16 mt + (l & 15) and of
// doc token 16 tile + (l & 15), and C/D of doc column l & 15 for the query rows 16 mt + 4 (l >> 4) + i; the K steps go
// in ascending order into one accumulator per (mt, tile).  A C element depends on its own A row and B column alone, so
// every element sees the same instruction sequence on the same values as in k_maxsim; the maximum is order-free and the
// sum over the query's tokens has one order.
//
// k_tok_scores<P, MT> (MT = the query's tiles of 16 tokens).  A persistent grid of four-wave blocks.  The query is staged
// ONCE per block, straight into registers: a lane's A fragments are MT * P / 32 * 16 bytes (64 VGPRs at MT = 4,
// P = 128) and are read by every MFMA of the kernel, which an LDS copy would re-read at one ds_read_b128 per MFMA.
// Block b takes the runs of 4 * per consecutive rows b, b + grid, ...; wave w of the block takes the `per` <= 16 rows
// per * w .. per * w + per - 1 of the run (its "turn"): lanes 0 .. per - 1 read the rows' offsets and allow bits, a
// masked, empty or matrix-less row is dropped from the turn's live set before any of its tokens is loaded, and the
// wave walks the 16-token tiles of the live docs as ONE sequence -- tiles never span docs; the last tile of a doc
// re-reads the doc's last token in the lanes beyond its end and enters -inf for them.  `per` is 16 for a scan (few
// turns per wave would leave the prefetch nothing to run ahead into) and smaller where the rows are few, so that a
// re-rank of 64 rows runs on 64 waves and not on 4.
// The doc fragments of tile i + 2 are loaded (16-byte non-temporal loads straight to VGPRs: every byte is used once by
// one wave) before the MFMAs of tile i, across doc boundaries, through three register buffers used in turn (no copies
// between them, so a wait is for one tile's loads only).  At the end of
// a doc the running maxima are reduced over the 16 lanes of a row group with DPP (row16_allmax) and PARKED in the
// wave's LDS rows [16][65]; at the end of the turn lane d < per adds doc d's maxima in ascending query token, so the
// chains of up to 64 dependent adds of 16 docs run side by side once per turn, not once per doc, and the wave stores
// `per` consecutive floats of the column.  No atomics and no cross-wave traffic: the bits do not depend on the grid.
// Rows come from `rows` (a list of n row numbers: css_index_maxsim_rows) or are 0 .. n - 1 (rows == null).
// Traffic: 2 P bytes per stored token of an allowed row, 16 bytes of offsets and 4 of column per row.
#pragma once

constexpr int kTokQ = 64;             // query tokens at most (CSS_MAX_QUERY_TOKENS)
constexpr int kTokTurn = 16;          // docs of one wave's turn
constexpr int kTokPark = kTokQ + 1;   // floats between two docs' parked maxima: odd, the adding lanes hit distinct banks
typedef short tok_v8s __attribute__((ext_vector_type(8)));

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

template <int P, int MT>
__global__ __launch_bounds__(64 * kWaves) void k_tok_scores(const unsigned short* __restrict__ tok,
                                                            const int64_t* __restrict__ off, int64_t nlist,
                                                            const uint32_t* __restrict__ rows, int64_t n,
                                                            const uint32_t* __restrict__ mask,
                                                            const unsigned short* __restrict__ q, int mq, int per,
                                                            float* __restrict__ col) {
    static_assert(P % 32 == 0 && P >= 32 && P <= 128, "whole K steps of the MFMA");
    static_assert(MT >= 1 && MT * 16 <= kTokQ, "the query's tiles");
    constexpr int KS = P / 32;
    __shared__ float park[kWaves][kTokTurn * kTokPark];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const float ninf = -__builtin_inff();
    // the query, once: rows beyond it inside its last tile are zeros, their results are never read
    v8bf qa[MT][KS];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int r = 16 * mt + lr;
            const uint4 v = r < mq ? *reinterpret_cast<const uint4*>(q + (size_t)r * P + 32 * ks + 8 * g) : make_uint4(0u, 0u, 0u, 0u);
            qa[mt][ks] = __builtin_bit_cast(v8bf, v);
        }
    float* mypark = park[wave];
    const int64_t nturns = (n + per - 1) / per;   // (1 <= per <= kTokTurn)
    for (int64_t turn = (int64_t)blockIdx.x * kWaves + wave; turn < nturns; turn += (int64_t)gridDim.x * kWaves) {
        const int64_t pos = turn * per + lr;
        int md_lane = 0;
        int64_t beg_lane = 0;
        if (lane < per && pos < n) {
            const int64_t row = rows != nullptr ? (int64_t)rows[pos] : pos;
            if (row < nlist && (mask == nullptr || ((mask[row >> 5] >> (row & 31)) & 1u))) {
                beg_lane = off[row];
                md_lane = (int)(off[row + 1] - beg_lane);
            }
        }
        TokAt ld;   // the next tile to load ...
        ld.live = (unsigned)__ballot(lane < per && md_lane > 0);
        tok_next_doc(ld, md_lane, beg_lane);
        TokAt at = ld;   // ... and the next to multiply
        tok_v8s b0[KS], b1[KS], b2[KS];
        auto load = [&](tok_v8s(&b)[KS]) {
            if (ld.j >= kTokTurn) return;
            const unsigned short* drow = tok + ((size_t)ld.beg + (size_t)min(ld.t * 16 + lr, ld.md - 1)) * P + 8 * g;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = __builtin_nontemporal_load(reinterpret_cast<const tok_v8s*>(drow + 32 * ks));
            tok_next_tile(ld, md_lane, beg_lane);
        };
        v4f run[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) run[mt] = v4f{ninf, ninf, ninf, ninf};
        // tile i of the sequence sits in buffer i % 3; its step first loads tile i + 2 into the buffer of tile i - 1
        auto step = [&](tok_v8s(&cur)[KS], tok_v8s(&nxt)[KS]) {
            load(nxt);
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
                for (int i = 0; i < 4; ++i) run[mt][i] = fmaxf(run[mt][i], ok ? acc[mt][i] : ninf);
            const int doc = at.j;
            tok_next_tile(at, md_lane, beg_lane);
            if (at.j == doc) return;
            // the doc's last tile: its maxima are parked for the adds at the end of the turn
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
        while (true) {
            if (at.j >= kTokTurn) break;
            step(b0, b2);
            if (at.j >= kTokTurn) break;
            step(b1, b0);
            if (at.j >= kTokTurn) break;
            step(b2, b1);
        }
        // (one wave writes and reads its own LDS rows: the LDS keeps a wave's accesses in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < per && pos < n) {
            float s = ninf;
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
}

// The matrix mover of css_index_remove_rows, one wave per source row r < nlist: a kept row's tokens move to token
// noff[map[r]] of the new buffer (map[r] = the row's new number, kLexNoRow when it goes).  u4 = P / 8: the 16-byte
// pieces of a token.
__global__ __launch_bounds__(256) void k_tok_move(const uint4* __restrict__ tok, const int64_t* __restrict__ off,
                                                  const uint32_t* __restrict__ map, const int64_t* __restrict__ noff,
                                                  int64_t nlist, int u4, uint4* __restrict__ ntok) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= nlist) return;
    const uint32_t nr = map[r];
    if (nr == kLexNoRow) return;
    const int64_t s = off[r] * u4, cnt = (off[r + 1] - off[r]) * u4, d = noff[nr] * u4;
    for (int64_t i = lane; i < cnt; i += 64) ntok[d + i] = tok[s + i];
}
