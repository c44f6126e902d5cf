// css_kmeans.h -- one Lloyd step on the flat index: every allowed row is assigned to its nearest centroid and the
// members of every centroid are summed, on the device, next to the rows.
// Included by css_index.hip (inside its anonymous namespace, after k_scan_mfma: it reuses MF_BM / MF_BN / MF_BK,
// mf_swz, f32x16 and v4f).  include/css_hip.h (css_index_kmeans_step) states the rules; this file says how.
//
// k_kmeans_assign is the K loop of k_scan_mfma with the operands swapped: the CENTROIDS are the A operand and the
// ROWS the B operand of v_mfma_f32_32x32x2_f32, so a lane holds the scores of ONE row (column fr of its wave's 32
// rows) against 64 of the 128 centroids of the tile, and lane fr + 32 holds the other 64.  The argmax over a
// centroid tile is 64 compares in registers, the two halves meet in one shuffle, and because a wave owns all 128
// centroids of its 32 rows nothing crosses waves: there is no list, no threshold exchange and no pacing.  A block
// owns a strip of row tiles and walks every centroid tile for each of them; the table ([ncpad][dpad], at most
// 12.6 MB) stays in L2 / Infinity Cache.  Staging (global -> registers -> swizzled LDS, double buffered, one barrier
// per K-step) is k_scan_mfma's.
//     key(r, c) = fmaf(-0.5f, ||c||^2, <x_r, c>)      a(r) = argmax_c key, ties to the lower c
//     dist(r)   = fmaxf(0, fmaf(-2, key, xnorm2[r]))
// Within a lane the centroid numbers of the 64 registers ascend with (m, r), and the tiles ascend, so a strict
// `>` keeps the lowest index; the two lane halves are merged on (key, index).  Pad centroids c >= nc carry
// ||c||^2 = +inf: their key is -inf and never wins.  (The table of norms keeps ||c||^2, not its half: fmaf(-0.5f, n2, s)
// is the stated rule bit for bit also where n2 / 2 would be subnormal.)
// The per-centroid member counts are taken in LDS (one 32-bit LDS atomic per row) and flushed once per block with
// 64-bit global atomics; the objective llrint(dist * 2^t) is summed per wave over the whole strip and added once.
//
// Member lists: k_kmeans_offsets (one block) turns the counts into offsets and into the block numbers of
// k_kmeans_sum (one block per centroid and segment of KM_SEG members); k_kmeans_members appends row numbers through
// one cursor per centroid.  The order inside a list is whatever it comes out as.
//
// k_kmeans_sum: a thread owns the float4 column chunks tid, tid + 256, ...; it reads its members' rows in place
// (16 bytes per lane, consecutive lanes consecutive chunks), accumulates llrint(x * 2^s) in int64 registers and
// flushes one 64-bit atomic per column.  Integer sums: the result is the same whatever order the atomics land in.
// There is no float atomic, no sort and no per-block [nc][d] table anywhere in the step.
#pragma once

constexpr int KM_SEG = 1024;   // members per block of k_kmeans_sum
// int64 words in front of the counts and sums of a step (km_out): [0] objective, [1] s, [2] t, [3] s is safe,
// [4] the largest safe s, [5] bits of the double 2^s, [6] bits of the double 2^t, [7] unused
constexpr int KM_HDR = 8;

// The shift rule of css_index_kmeans_step (flat_index.kmeans_shift restates it), evaluated on the device so that the
// call needs no readback in front of its launches: ex = frexp(max ||x||^2), e = ceil(ex / 2), b = bit_length(n - 1),
// s = 62 - b - e unless the caller imposes one, t = s - e - 2.
__global__ void k_kmeans_params(const int* __restrict__ maxn2, int64_t n, int fx_shift, long long* __restrict__ hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float m = __int_as_float(maxn2[0]);
    int ex = 0;
    if (m > 0.f) (void)frexpf(m, &ex);
    const int e = (ex + 1) >> 1;   // ceil(ex / 2) for either sign
    const unsigned long long v = (unsigned long long)(n > 1 ? n : 1) - 1ull;
    const int b = v ? 64 - __clzll((long long)v) : 0;
    const int safe = 62 - b - e;
    const int s = fx_shift >= 0 ? fx_shift : safe;
    const int t = s - e - 2;
    hdr[0] = 0;
    hdr[1] = s;
    hdr[2] = t;
    hdr[3] = s <= safe ? 1 : 0;
    hdr[4] = safe;
    hdr[5] = __double_as_longlong(ldexp(1.0, s));
    hdr[6] = __double_as_longlong(ldexp(1.0, t));
    hdr[7] = 0;
}

// The K loop of k_kmeans_assign and k_transform_rows (css_pca.h): a block walks its strip of 128-row tiles, and for each
// of them every 128-row tile of the table `ctab` ([nctiles * 128][dpad]: the A operand), accumulating the 128 x 128
// scores on the fp32-input matrix core.  What happens to the scores is the epilogue's:
//     epi.init(lds, tid)            once, in front of the first barrier; `lds` is the dynamic LDS behind As / Bs
//     epi.tile(acc, ct, row, fh)    after the last K-step of table tile ct: acc[m][r] is the score of THIS lane's row
//                                   `row` (it may be >= ntotal) against table row ct * 128 + 32 m + (r & 3) + 8 (r >> 2)
//                                   + 4 fh; the epilogue leaves acc zeroed
// Returns false, having touched nothing, when the block has no tile.
template <class Epi>
__device__ __forceinline__ bool km_sweep(const float* __restrict__ xb, const float* __restrict__ ctab, int nctiles,
                                         int64_t ntotal, int dpad, int64_t tiles_per_block, char* smem, Epi& epi) {
    float* As = reinterpret_cast<float*>(smem);
    float* Bs = As + 2 * MF_BM * MF_BK;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ntiles = (ntotal + MF_BN - 1) / MF_BN;
    const int64_t t_begin = (int64_t)blockIdx.x * tiles_per_block;
    const int64_t t_end = min(t_begin + tiles_per_block, ntiles);
    if (t_begin >= t_end) return false;
    epi.init(Bs + 2 * MF_BN * MF_BK, tid);

    const int KT = dpad / MF_BK;
    const int64_t n_it = (t_end - t_begin) * nctiles * KT;
    const int srow = tid >> 3, schunk = tid & 7;
    v4f ra[4], rb[4];

#define KM_GLOAD(RT, CT, KT_)                                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        int64_t row_ = (RT) * MF_BN + srow + 32 * i;                                                         \
        row_ = row_ < ntotal ? row_ : ntotal - 1;                                                            \
        ra[i] = *reinterpret_cast<const v4f*>(ctab + (int64_t)((CT) * MF_BM + srow + 32 * i) * dpad +        \
                                              (KT_) * MF_BK + schunk * 4);                                   \
        rb[i] = *reinterpret_cast<const v4f*>(xb + row_ * (int64_t)dpad + (KT_) * MF_BK + schunk * 4);       \
    }
#define KM_SSTORE(BUF)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        *reinterpret_cast<v4f*>(As + (BUF) * MF_BM * MF_BK + mf_swz(srow + 32 * i, schunk)) = ra[i];         \
        *reinterpret_cast<v4f*>(Bs + (BUF) * MF_BN * MF_BK + mf_swz(srow + 32 * i, schunk)) = rb[i];         \
    }

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    const int jr = wave * 32 + fr;   // this lane's row inside the row tile

    KM_GLOAD(t_begin, 0, 0)
    KM_SSTORE(0)
    __syncthreads();   // (also orders what epi.init wrote)
    int cur = 0;
    int64_t rt = t_begin;
    int ct = 0, kt = 0;
    for (int64_t it = 0; it < n_it; ++it) {
        if (it + 1 < n_it) {
            int nkt = kt + 1, nct = ct;
            int64_t nrt = rt;
            if (nkt == KT) {
                nkt = 0;
                if (++nct == nctiles) {
                    nct = 0;
                    ++nrt;
                }
            }
            KM_GLOAD(nrt, nct, nkt)
        }
        const float* A = As + cur * MF_BM * MF_BK;
        const float* B = Bs + cur * MF_BN * MF_BK;
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // 8 k-values per chunk pair: lane half fh takes chunk 2c+fh
            const v4f b = *reinterpret_cast<const v4f*>(B + mf_swz(jr, 2 * c + fh));
            v4f a[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = *reinterpret_cast<const v4f*>(A + mf_swz(32 * m + fr, 2 * c + fh));
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].x, b.x, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].y, b.y, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].z, b.z, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].w, b.w, acc[m], 0, 0, 0);
            }
        }
        if (kt == KT - 1) epi.tile(acc, ct, rt * MF_BN + jr, fh);
        if (it + 1 < n_it) {
            KM_SSTORE(cur ^ 1)
        }
        __syncthreads();
        cur ^= 1;
        if (++kt == KT) {
            kt = 0;
            if (++ct == nctiles) {
                ct = 0;
                ++rt;
            }
        }
    }
#undef KM_GLOAD
#undef KM_SSTORE
    return true;
}

// The epilogue of k_kmeans_assign: the running argmax of this lane's row over the table tiles, and at the last tile
// the row's assignment, distance, LDS member count and objective term.
struct KmAssignEpi {
    const float* __restrict__ xnorm2;
    const float* __restrict__ cn2;
    int nc, nctiles;
    int64_t ntotal;
    const uint32_t* __restrict__ mask;
    double scale_t;
    int32_t* __restrict__ assign;
    float* __restrict__ dist;
    float* cn2s;
    unsigned int* cnt;
    float bkey;
    int bc;
    long long objw;
    __device__ __forceinline__ void init(float* lds, int tid) {
        cn2s = lds;
        cnt = reinterpret_cast<unsigned int*>(cn2s + nctiles * MF_BM);
        for (int i = tid; i < nctiles * MF_BM; i += 256) cn2s[i] = cn2[i];
        for (int i = tid; i < nc; i += 256) cnt[i] = 0u;
    }
    __device__ __forceinline__ void tile(f32x16 (&acc)[4], int ct, int64_t row, int fh) {
        // ---------------- the 64 keys of this lane's row against centroid tile ct, ascending centroid number
        const int cbase = ct * MF_BM;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = cbase + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * fh;
                const float key = fmaf(-0.5f, cn2s[c], acc[m][r]);
                if (key > bkey) {
                    bkey = key;
                    bc = c;
                }
                acc[m][r] = 0.f;
            }
        if (ct != nctiles - 1) return;
        // ---------------- the row is done: the two lane halves meet, lane fr of half 0 writes it
        const float okey = __shfl_xor(bkey, 32);
        const int oc = __shfl_xor(bc, 32);
        if (okey > bkey || (okey == bkey && oc < bc)) {
            bkey = okey;
            bc = oc;
        }
        if (fh == 0 && row < ntotal) {
            const bool ok = mask == nullptr || ((mask[row >> 5] >> (row & 31)) & 1u);
            int a_r = -1;
            float d_r = 0.f;
            if (ok) {
                a_r = bc;
                d_r = fmaxf(0.f, fmaf(-2.f, bkey, xnorm2[row]));
                atomicAdd(&cnt[bc], 1u);
                objw += (long long)rint((double)d_r * scale_t);
            }
            assign[row] = a_r;
            dist[row] = d_r;
        }
        bkey = -INFINITY;
        bc = 0;
    }
};

// LDS: As [2][128][32] centroids | Bs [2][128][32] rows | cn2s [ncpad] | cnt [nc]
__global__ __launch_bounds__(256, 2) void k_kmeans_assign(const float* __restrict__ xb, const float* __restrict__ xnorm2,
                                                          const float* __restrict__ ctab, const float* __restrict__ cn2,
                                                          int nc, int nctiles, int64_t ntotal, int dpad,
                                                          int64_t tiles_per_block, const uint32_t* __restrict__ mask,
                                                          const long long* __restrict__ hdr, int32_t* __restrict__ assign,
                                                          float* __restrict__ dist, unsigned long long* __restrict__ counts,
                                                          unsigned long long* __restrict__ obj) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    KmAssignEpi epi{xnorm2, cn2, nc, nctiles, ntotal, mask, __longlong_as_double(hdr[6]), assign, dist,
                    nullptr, nullptr, -INFINITY, 0, 0};
    if (!km_sweep(xb, ctab, nctiles, ntotal, dpad, tiles_per_block, smem, epi)) return;
    long long objw = epi.objw;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) objw += __shfl_xor(objw, off);
    if (lane == 0 && objw != 0) atomicAdd(obj, (unsigned long long)objw);
    // (the barrier that closed the last K-step is behind every LDS count)
    for (int i = tid; i < nc; i += 256)
        if (epi.cnt[i]) atomicAdd(counts + i, (unsigned long long)epi.cnt[i]);
}

// One block: counts -> exclusive offsets off[0..nc] into the member lists and seg[0..nc], the exclusive prefix of
// ceil(count / KM_SEG): block b of k_kmeans_sum serves the centroid c with seg[c] <= b < seg[c + 1].  nc <= 4096.
__global__ __launch_bounds__(1024) void k_kmeans_offsets(const unsigned long long* __restrict__ counts, int nc,
                                                         uint32_t* __restrict__ off, uint32_t* __restrict__ seg) {
    __shared__ uint32_t so[1024], ss[1024];
    const int tid = threadIdx.x;
    uint32_t c[4], g[4], tc = 0, tg = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid * 4 + j;
        c[j] = i < nc ? (uint32_t)counts[i] : 0u;
        g[j] = (c[j] + KM_SEG - 1) / KM_SEG;
        tc += c[j];
        tg += g[j];
    }
    so[tid] = tc;
    ss[tid] = tg;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t a = tid >= d ? so[tid - d] : 0u, b = tid >= d ? ss[tid - d] : 0u;
        __syncthreads();
        so[tid] += a;
        ss[tid] += b;
        __syncthreads();
    }
    uint32_t eo = so[tid] - tc, eg = ss[tid] - tg;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid * 4 + j;
        if (i < nc) {
            off[i] = eo;
            seg[i] = eg;
        }
        eo += c[j];
        eg += g[j];
    }
    if (tid == 1023) {
        off[nc] = so[1023];
        seg[nc] = ss[1023];
    }
}

// One thread per row: its number appended to the list of its centroid.
__global__ __launch_bounds__(256) void k_kmeans_members(const int32_t* __restrict__ assign, int64_t ntotal,
                                                        const uint32_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                        uint32_t* __restrict__ members) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= ntotal) return;
    const int a = assign[r];
    if (a < 0) return;
    members[off[a] + atomicAdd(cursor + a, 1u)] = (uint32_t)r;
}

__device__ __forceinline__ void km_acc4(long long (&s)[4], const float4 v, double scale) {
    s[0] += (long long)rint((double)v.x * scale);
    s[1] += (long long)rint((double)v.y * scale);
    s[2] += (long long)rint((double)v.z * scale);
    s[3] += (long long)rint((double)v.w * scale);
}

// One block per (centroid, segment of at most KM_SEG members); grid = nc + ceil(ntotal / KM_SEG) >= seg[nc].
__global__ __launch_bounds__(256) void k_kmeans_sum(const float4* __restrict__ xb, const uint32_t* __restrict__ members,
                                                    const uint32_t* __restrict__ off, const uint32_t* __restrict__ seg,
                                                    int nc, int dim, int dpad4, const long long* __restrict__ hdr,
                                                    unsigned long long* __restrict__ sums) {
    const uint32_t b = blockIdx.x;
    if (b >= seg[nc]) return;
    int lo = 0, hi = nc;   // the last c in [0, nc) with seg[c] <= b (empty centroids share a value with their successor)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int c = lo;
    const uint32_t begin = off[c] + (b - seg[c]) * KM_SEG;
    const uint32_t end = min(begin + (uint32_t)KM_SEG, off[c + 1]);
    const double scale = __longlong_as_double(hdr[5]);
    for (int q = threadIdx.x; q < dpad4; q += 256) {
        long long s[4] = {0, 0, 0, 0};
        uint32_t i = begin;
        for (; i + 4 <= end; i += 4) {   // four rows in flight
            const float4 v0 = xb[(size_t)members[i] * dpad4 + q], v1 = xb[(size_t)members[i + 1] * dpad4 + q];
            const float4 v2 = xb[(size_t)members[i + 2] * dpad4 + q], v3 = xb[(size_t)members[i + 3] * dpad4 + q];
            km_acc4(s, v0, scale);
            km_acc4(s, v1, scale);
            km_acc4(s, v2, scale);
            km_acc4(s, v3, scale);
        }
        for (; i < end; ++i) km_acc4(s, xb[(size_t)members[i] * dpad4 + q], scale);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < dim && s[j] != 0) atomicAdd(sums + (size_t)c * dim + 4 * q + j, (unsigned long long)s[j]);
    }
}
