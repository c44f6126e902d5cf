// css_pca.h -- the two device primitives of PCA on the flat index: the fixed-point second-moment (Gram) matrix of the
// stored rows with their column sums, and y = A x + b over a range of stored rows.
// Included by css_index.hip (inside its anonymous namespace, after css_kmeans.h: k_transform_rows is the K loop of
// k_kmeans_assign, km_sweep, under another epilogue).  include/css_hip.h (css_index_gram, css_index_transform) states
// the rules; this file says how.
//
// k_gram_fx: G = Q^T Q with q = rint((double)x * 2^p), on the fp64 matrix core (v_mfma_f64_16x16x4_f64).  The stored
// ROWS are the K dimension.  A block owns one 128 x 128 tile (ti <= tj) of the upper tile triangle of the padded
// matrix and one strip of rows; its four waves own the 64 x 64 quarters, 16 MFMA tiles of 4 doubles per lane.
//   staging   16 rows x (128 columns of panel ti | 128 columns of panel tj) per chunk: global float4 -> registers ->
//             quantised -> LDS, double buffered, one barrier per chunk (the scheme of k_kmeans_assign).  |q| <= 2^20 is
//             an integer below 2^24, so it is kept in LDS as a FLOAT without loss: half the bytes of a double, and the
//             conversion back (v_cvt_f64_f32) is exact.  A row that is masked out, or past the strip, is staged as zeros.
//   operands  lane l of a K-step of 4 rows reads ONE float4 per panel: row (l >> 4), columns 4 (l & 15) + {0,1,2,3} of
//             its wave's 64.  Element a of that float4 is the A (or B) operand of MFMA tile a, so tile (a, b) holds the
//             products of columns 4 i + a and 4 j + b: a permutation of the 64 x 64 quarter, undone at the flush.
//             A / B lane maps are those of the f32 16x16x4 form; C / D is col = l & 15, row = (l >> 4) + 4 * reg.
//   the fold  |q| <= 2^20 (the shift rule), so a product is an integer of at most 2^40 and a partial sum over at most
//             GR_FOLD = 8192 = 2^13 rows an integer of at most 2^53: every intermediate value is an integer that a
//             double holds exactly, so each accumulation step is exact whatever the order inside the matrix core.  One
//             row more and that no longer holds.  So after every 8192 rows the 64 doubles of a lane are added into 64
//             int64 registers and cleared.  8192 is this derivation, not a tuning knob.
//   the flush once per block, 64-bit INTEGER vector atomics (global_atomic_add_x2): the result does not depend on the
//             order they land in, nor on the grid.  The lower tile triangle is never written; the host mirrors it.
//   colsum    in the diagonal tiles: the thread that quantises a float4 of panel ti always serves the same 4 columns,
//             so it keeps their 4 integer sums in registers and flushes them with the same atomics.
// No float atomics, no scalar-unit stores.
#pragma once

constexpr int GR_T = 128;       // edge of an output tile
constexpr int GR_KC = 16;       // rows per staged chunk (4 K-steps of the 16x16x4 form)
constexpr int GR_FOLD = 8192;   // rows between two folds of the fp64 accumulators into int64 (derived above)
// int64 words in front of the column sums and the matrix (gr_out): [0] p, [1] p is safe, [2] the largest safe p,
// [3] bits of the double 2^p
constexpr int GR_HDR = 4;
typedef double f64x4 __attribute__((ext_vector_type(4)));

// The shift rule of css_index_gram (flat_index.pca_shift restates it), on the device as k_kmeans_params:
// p = min(20, (62 - b) >> 1) - e unless the caller imposes one.
__global__ void k_gram_params(const int* __restrict__ maxn2, int64_t n, int fx_shift, long long* __restrict__ hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float m = __int_as_float(maxn2[0]);
    int ex = 0;
    if (m > 0.f) (void)frexpf(m, &ex);
    const int e = (ex + 1) >> 1;   // ceil(ex / 2) for either sign
    const unsigned long long v = (unsigned long long)(n > 1 ? n : 1) - 1ull;
    const int b = v ? 64 - __clzll((long long)v) : 0;
    const int half = (62 - b) >> 1;
    const int safe = (half < 20 ? half : 20) - e;
    const int p = fx_shift >= 0 ? fx_shift : safe;
    hdr[0] = p;
    hdr[1] = p <= safe ? 1 : 0;
    hdr[2] = safe;
    hdr[3] = __double_as_longlong(ldexp(1.0, p));
}

// grid.x: the tiles (ti <= tj) of the upper triangle of (gp / 128)^2, row-major; grid.y: strips of rows_per_block rows
// (a multiple of GR_KC).  G is [gp][gp], colsum [gp]; gp = dpad rounded up to 128, columns >= dpad are staged as zeros.
__global__ __launch_bounds__(256, 1) void k_gram_fx(const float* __restrict__ xb, int64_t ntotal, int dpad, int gp,
                                                    int64_t rows_per_block, const uint32_t* __restrict__ mask,
                                                    const long long* __restrict__ hdr, unsigned long long* __restrict__ G,
                                                    unsigned long long* __restrict__ colsum) {
    __shared__ __attribute__((aligned(16))) float Qs[2][GR_KC][2 * GR_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = gp / GR_T;
    int ti = 0, t = (int)blockIdx.x;
    while (t >= T - ti) {
        t -= T - ti;
        ++ti;
    }
    const int tj = ti + t;
    const int64_t r_begin = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r_end = min(r_begin + rows_per_block, ntotal);
    if (r_begin >= r_end) return;
    const double scale = __longlong_as_double(hdr[3]);

    // staging: thread = float4 chunk schunk of the 256 staged columns (0..31 panel ti, 32..63 panel tj), rows srow + 4 i
    const int schunk = tid & 63, srow = tid >> 6;
    const int scol = (schunk < 32 ? ti : tj) * GR_T + (schunk & 31) * 4;   // the column in the stored rows
    const bool col_ok = scol < dpad;                                       // (dpad is a multiple of 64: all four or none)
    const bool sums = ti == tj && schunk < 32;                             // this thread forms 4 column sums
    const float* src = xb + (col_ok ? scol : 0);
    long long cs[4] = {0, 0, 0, 0};
    v4f rq[4];

#define GR_GLOAD(CH)                                                                                         \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        const int64_t row_ = r_begin + (int64_t)(CH) * GR_KC + srow + 4 * i;                                 \
        const int64_t rr_ = row_ < r_end ? row_ : r_end - 1;                                                 \
        const bool ok_ = col_ok && row_ < r_end && (mask == nullptr || ((mask[rr_ >> 5] >> (rr_ & 31)) & 1u)); \
        const v4f v_ = *reinterpret_cast<const v4f*>(src + rr_ * (int64_t)dpad);                             \
        rq[i] = ok_ ? v_ : v4f{0.f, 0.f, 0.f, 0.f};                                                          \
    }
#define GR_SSTORE(BUF)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        const double q0_ = __builtin_rint((double)rq[i].x * scale), q1_ = __builtin_rint((double)rq[i].y * scale); \
        const double q2_ = __builtin_rint((double)rq[i].z * scale), q3_ = __builtin_rint((double)rq[i].w * scale); \
        if (sums) {                                                                                          \
            cs[0] += (long long)(int)q0_;                                                                    \
            cs[1] += (long long)(int)q1_;                                                                    \
            cs[2] += (long long)(int)q2_;                                                                    \
            cs[3] += (long long)(int)q3_;                                                                    \
        }                                                                                                    \
        *reinterpret_cast<v4f*>(&Qs[BUF][srow + 4 * i][schunk * 4]) = v4f{(float)q0_, (float)q1_, (float)q2_, (float)q3_}; \
    }

    f64x4 acc[4][4];
    long long iacc[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) iacc[a][b][r] = 0;
        }

    const int li = lane & 15, lk = lane >> 4;
    const int wi = wave >> 1, wj = wave & 1;
    const int acol = 64 * wi + 4 * li, bcol = GR_T + 64 * wj + 4 * li;   // this lane's float4 in either panel
    const int64_t nchunks = (r_end - r_begin + GR_KC - 1) / GR_KC;
    int since_fold = 0;

    GR_GLOAD(0)
    GR_SSTORE(0)
    __syncthreads();
    int cur = 0;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks) {
            GR_GLOAD(ch + 1)
        }
#pragma unroll
        for (int s = 0; s < GR_KC / 4; ++s) {
            const v4f fa = *reinterpret_cast<const v4f*>(&Qs[cur][4 * s + lk][acol]);
            const v4f fb = *reinterpret_cast<const v4f*>(&Qs[cur][4 * s + lk][bcol]);
            const double da[4] = {(double)fa.x, (double)fa.y, (double)fa.z, (double)fa.w};
            const double db[4] = {(double)fb.x, (double)fb.y, (double)fb.z, (double)fb.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[a], db[b], acc[a][b], 0, 0, 0);
        }
        since_fold += GR_KC;
        if (since_fold == GR_FOLD || ch + 1 == nchunks) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        iacc[a][b][r] += (long long)acc[a][b][r];
                        acc[a][b][r] = 0.0;
                    }
            since_fold = 0;
        }
        if (ch + 1 < nchunks) {
            GR_SSTORE(cur ^ 1)
        }
        __syncthreads();
        cur ^= 1;
    }
#undef GR_GLOAD
#undef GR_SSTORE
    // D of tile (a, b): row (lk + 4 r) is column 4 (lk + 4 r) + a of the wave's rows of G, col li is column 4 li + b
    const int gi0 = ti * GR_T + 64 * wi, gj0 = tj * GR_T + 64 * wj;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long v = iacc[a][b][r];
                if (v != 0)
                    atomicAdd(G + (size_t)(gi0 + 4 * (lk + 4 * r) + a) * gp + (gj0 + 4 * li + b), (unsigned long long)v);
            }
    if (sums) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cs[j] != 0) atomicAdd(colsum + scol + j, (unsigned long long)cs[j]);
    }
}

// The epilogue of k_transform_rows under km_sweep: the table is A (row c of the table = row c of A), and the 64 scores
// of this lane's row against a table tile are written as y[row][c] = score + b[c] for c < m.  Nothing crosses lanes.
struct TransformEpi {
    const float* __restrict__ bias;   // [nctiles * 128]
    float* __restrict__ y;            // [ntotal, m]
    int m, nctiles;
    int64_t ntotal;
    float* bs;
    __device__ __forceinline__ void init(float* lds, int tid) {
        bs = lds;
        for (int i = tid; i < nctiles * MF_BM; i += 256) bs[i] = bias[i];
    }
    __device__ __forceinline__ void tile(f32x16 (&acc)[4], int ct, int64_t row, int fh) {
        const int cbase = ct * MF_BM;
#pragma unroll
        for (int mm = 0; mm < 4; ++mm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cbase + 32 * mm + (r & 3) + 8 * (r >> 2) + 4 * fh;
                if (row < ntotal && c < m) y[row * (int64_t)m + c] = acc[mm][r] + bs[c];
                acc[mm][r] = 0.f;
            }
    }
};

// LDS: As [2][128][32] rows of A | Bs [2][128][32] stored rows | bs [nctiles * 128]
__global__ __launch_bounds__(256, 2) void k_transform_rows(const float* __restrict__ xb, const float* __restrict__ atab,
                                                           const float* __restrict__ bias, int m, int nctiles,
                                                           int64_t ntotal, int dpad, int64_t tiles_per_block,
                                                           float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TransformEpi epi{bias, y, m, nctiles, ntotal, nullptr};
    (void)km_sweep(xb, atab, nctiles, ntotal, dpad, tiles_per_block, smem, epi);
}
