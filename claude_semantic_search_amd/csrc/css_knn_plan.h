// css_knn_plan.h -- the rules of the candidate cascade as plain C++: which kind of cascade a call is, its growth factor,
// its schedule of stages, the a-priori error bound of its coarse scores and the ticket table of the one-launch sweep.
// Standard headers only: a host compiler builds it alone (tests/native/cascade_plan.cc), css_index.hip applies it
// (launch_scan_coarse), css_knn_coarse.h holds the kernels it schedules.
#pragma once

#include <cmath>
#include <cstdint>

// stages that k_sweep_cascade (the 1..4-query cascade in one launch) can hold: the size of its ticket table and of its
// state words (growth 4: 4^15 tiles)
constexpr int CZ_FS_MAXST = 16;

enum class CascadeKind {
    Batch,       // query tiles of 256 on the MFMA scan (k_scan_coarse8 / k_scan_coarse, int8 rows: k_scan_qreg_i8)
    SweepValu,   // 1..4 queries on the HBM-bound VALU sweep (k_sweep_coarse / _i8, or all stages as k_sweep_cascade)
    SweepMfma,   // 3..32 queries on the int8-MFMA sweep (k_sweep_mfma_i8): int8 rows and int8 queries
};

// Growth factor g: every stage reads g-1 times the tiles read before it.  Batches (MFMA scan): g = 8 for k <= 32
// (4 stages at 1.25 M rows instead of 6; the last stage is 7/8 of the rows and appends ~7k + band candidates per
// query, cheap since the tile epilogue walks hits per lane: 10 M x 1000, k = 10: 12.25 ms vs 12.47 at g = 4, 100 k
// rows 0.32 vs 0.34 ms; g = 16: 12.4 ms), g = 4 above (k = 100: 13.55 vs 13.79 ms; k = 32..64 equal).  Round 2's
// epilogue made g = 8 2 % slower.  1..4 queries (sweep): g = 4.  Fewer, larger stages do not help
// there -- measured at 10 M rows, k = 10: g = 4 / 8 / 16 (7 / 5 / 4 stages) all take 2.71-2.72 ms, the call is the
// 15.36 GB of shadow rows at the sweep's bandwidth plus ~0.25 ms -- and with k = 100 (the reference's call shape)
// g = 16 overflows the 4096-slot buffers (~k g candidates per stage) and lands in the exact fix-up: 10 ms.
// (int8 scan: its band is ~4 x wider, growth 8 would append ~2500 rows per query in the main stage)
// (3..32 queries on the int8 MFMA: one launch per stage, so below ~4 M rows fewer, larger stages win -- ms at growth 4 / 8,
// k = 10: 1 M rows 0.33 / 0.27, 100 k rows 0.13 / 0.10, 10 M rows 1.59 / 1.55-1.67; k = 100 overflows the buffers at
// growth 8 and 10 M rows, as the VALU sweep did)
// env_growth / env_growth_sweep: CSS_KNN_GROWTH / CSS_KNN_GROWTH_SWEEP (0: by shape).
inline int cascade_growth(CascadeKind kind, bool i8, int k, int64_t nrows, int env_growth, int env_growth_sweep) {
    if (kind == CascadeKind::Batch) return env_growth ? env_growth : ((k <= 32 && !i8) ? 8 : 4);
    return env_growth_sweep ? env_growth_sweep : ((kind == CascadeKind::SweepMfma && k <= 32 && nrows < 4000000) ? 8 : 4);
}

// Error of one coarse score relative to ||q|| max||x||, a priori: both operands bf16 (MFMA scan) or rows only (VALU sweep,
// fp32 queries).  int8 rows: |x^ - x| <= (s / 2) sqrt(d), s = max|x_i| / 127 <= ||x|| / 127 (the same for int8 queries).
// The 2^-11 covers the fp32 accumulation.  (cz_eps tightens it by the rounding errors measured at ingest / query prep.)
inline float cascade_eps_rel(CascadeKind kind, bool i8, int dpad) {
    const bool fp32_queries = kind == CascadeKind::SweepValu;
    const float i8_rel = sqrtf((float)dpad) / 254.f;
    return i8 ? (fp32_queries ? i8_rel : 2.f * i8_rel + i8_rel * i8_rel) + 0.00048828125f
              : (fp32_queries ? 0.00390625f + 0.00048828125f : 0.0078125f + 0.00048828125f);
}

// Which kinds fill stage 0 and split the last int8 step (the arguments of cascade_plan): not the VALU sweep, whose
// one-launch cascade of 1..2 queries has a first select of one wave's work (1.29 -> 1.32 ms with a fuller stage 0).
#ifndef CZ_S0_FILL
#define CZ_S0_FILL 1
#endif
inline bool cascade_fills_stage0(CascadeKind kind) { return CZ_S0_FILL && kind != CascadeKind::SweepValu; }
inline bool cascade_splits_last(CascadeKind kind, bool i8) { return i8 && kind != CascadeKind::SweepValu; }

// The schedule: a nested, uniformly strided sample of row tiles.  Stage 0 reads every tile at its stride (at most 15
// tiles: it keeps every score, 3840 of the 4096 slots), every later stage the tiles at a stride `ratio` times smaller
// that were not read before; the last stage has stride 1.
struct CascadeStage {
    int64_t stride;
    int ratio;       // stride of the previous stage / this stride (stage 0: unused)
    int64_t count;   // tiles the stage reads: all W = ceil(ntiles / stride) of stage 0, (W-1) - (W-1)/ratio afterwards
};
// (a stride per power of the growth >= 2 below 2^63 tiles, one coarser first stage, one split last step: no plan is longer)
constexpr int kCascadeMaxStages = CZ_FS_MAXST + 50;
struct CascadePlan {
    int64_t ntiles;
    int n;           // stages
    CascadeStage st[kCascadeMaxStages];
};
inline CascadePlan cascade_plan(int64_t ntiles, int growth, bool fill_stage0, bool split_last) {
    const int g = growth;
    CascadePlan p;
    p.ntiles = ntiles;
    p.n = 0;
    int64_t s0 = 1;
    while (ntiles / (s0 * g) >= 2) s0 *= g;
    // (2 .. 2g-1 tiles so far; stage 0 holds 15: where the next finer stride still fits, the cascade is one stage shorter --
    // batches 152.5 k -> 153.7 k queries/s, 4 / 16 queries on the int8 MFMA 1.67 / 1.72 -> 1.59 ms at 10 M rows)
    if (fill_stage0 && s0 >= g && (ntiles + s0 / g - 1) / (s0 / g) <= 15) s0 /= g;
    const int64_t w0 = (ntiles + s0 - 1) / s0;   // tiles at stride s0
    const int g0 = (int)((w0 + 14) / 15);        // > 1: one coarser first stage in front
    if (g0 > 1) p.st[p.n++] = {s0 * g0, 0, 0};
    p.st[p.n++] = {s0, g0, 0};
    for (int64_t s = s0 / g; s >= 1; s /= g) p.st[p.n++] = {s, g, 0};
    // int8 scan (band ~4 x wider): the last step of 4 is taken as two steps of 2 -- the main stage is then half of
    // the rows under the threshold of the other half (~3 x fewer appends than 3/4 of the rows under a quarter's)
    if (split_last && g == 4 && p.n >= 2 && p.st[p.n - 1].stride == 1 && ntiles >= 64) {
        p.st[p.n - 1] = {2, 2, 0};
        p.st[p.n++] = {1, 2, 0};
    }
    for (int si = 0; si < p.n; ++si) {
        const int64_t W = (ntiles + p.st[si].stride - 1) / p.st[si].stride;
        p.st[si].count = si == 0 ? W : (W - 1) - (W - 1) / p.st[si].ratio;
    }
    return p;
}
// what a stage's kernel gets to find its tiles: the u-th tile it reads is u + u / gm1 + 1 at its stride (stage 0 reads
// them all and takes the growth's: it does not use it)
inline int cascade_gm1(const CascadePlan& p, int growth, int si) {
    const int gm1 = (si == 0 ? growth : p.st[si].ratio) - 1;
    return gm1 > 1 ? gm1 : 1;
}

// The ticket table of the one-launch sweep (FsSched of css_knn_coarse.h): quarter tiles as tickets in stage order;
// first[n] = number of tickets.  False where the cascade has to stay one launch per stage: more stages than the table holds,
// tickets beyond an int, or a stage without tiles, which would leave nobody to run its select (not seen with these schedules).
inline bool cascade_tickets(const CascadePlan& p, int growth, int (&first)[CZ_FS_MAXST + 1], int (&stride)[CZ_FS_MAXST],
                            int (&gm1)[CZ_FS_MAXST]) {
    if (p.n > CZ_FS_MAXST || p.ntiles >= (int64_t)1 << 28) return false;
    int64_t next = 0;
    for (int si = 0; si < p.n; ++si) {
        if (p.st[si].count <= 0) return false;
        first[si] = (int)next;
        stride[si] = (int)p.st[si].stride;
        gm1[si] = cascade_gm1(p, growth, si);
        next += 4 * p.st[si].count;
    }
    first[p.n] = (int)next;
    return true;
}
