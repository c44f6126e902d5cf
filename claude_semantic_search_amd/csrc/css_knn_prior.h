// css_knn_prior.h -- prior-weighted search on the flat index: the k best rows under score + weight * prior[row].
// Included by css_index.hip (inside its anonymous namespace, after k_scan_small: it reuses scan_row_load and kWaves,
// and row16_allsum / wave_insert / f2key of css_knn_kernels.h).
//
// Retrieval stacks call the per-row term a function score, a rank-profile freshness term or a document prior.  It
// cannot be applied to an over-fetched list: a boosted row may sit anywhere below the fetched rows, so the fused value
// has to be the key of the sweep itself.
//
// k_scan_prior is the non-FIX sweep of k_scan_small with ONE change: behind row16_allsum the key of a row becomes the
// fused value
//     inner product   f = fmaf(weight, p_r, s)        larger is better, key = f
//     squared L2      f = fmaf(-weight, p_r, dist)    smaller is better, key = -f  (f may be negative)
// with p_r = prior[row] loaded once per row (HASP = false, an index without the column: 0, and no load).  Everything
// else is k_scan_small's: thread layout (block = 4 waves, a wave instruction covers 4 rows, 16 lanes x float4 per row
// and column step), queries in LDS, one
// fp32 fmaf chain per lane over the padded row, DPP row reduction, non-temporal row loads, the mask bit per row, the
// block-shared sorted lists (wave_insert), the grid-wide threshold gthr and the [q][block][k] part lists.  Keys are
// "larger is better" for both metrics, so k_merge_final<METRIC>, SweepGeom and grow_part serve unchanged
// (k_merge_final<L2> writes D = -key, which is f with its sign).  weight == 0 or no column give key == s bit for
// bit: fmaf(0, p, s) and fmaf(w, 0, s) are s for finite p and w (a chain that starts at +0 never ends at -0).
//
// The sweep body (row addressing, mask test, fmaf blocks) exists FIVE times on purpose: k_scan_small, k_range_small,
// here, k_scan_examples (css_knn_examples.h) and k_facet_small (css_knn_facets.h); css_knn_range.h and
// profiles/flat_index_refactor_shared_sweep_attempts.txt say why it is not one function.  A change to one is made to
// all five.
//
// The raw score.  The call also returns S, the row's own s / dist, so that thresholds keep their meaning.  A third
// LDS list beside keys and ids would cost NQ * k * 4 bytes of LDS per block and a third shifted array in every
// wave_insert of the slow path; instead k_prior_scores runs ONCE behind the merge and re-forms the scores of the nq * k
// returned rows with the very chain of the sweep (lane `sub` of a 16-lane row walks columns 64 t + 4 sub, t ascending,
// x y z w, then row16_allsum): the same operations in the same order on the same operands, hence the same bits --
// D == fmaf(+-weight, p, S) exactly.  The sweep stays at the register and LDS budget of k_scan_small.
#pragma once

template <int NQ, int TT, int METRIC, bool HASP>
__global__ __launch_bounds__(256, 4) void k_scan_prior(const float4* __restrict__ xb, const float* __restrict__ qpad,
                                                       int64_t ntotal, int T_rt, int k, int64_t groups_per_block,
                                                       int* __restrict__ gthr, float* __restrict__ part_s,
                                                       uint32_t* __restrict__ part_i, int nq_real,
                                                       const uint32_t* __restrict__ mask,
                                                       const float* __restrict__ prior, float weight) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = TT > 0 ? TT : T_rt;  // float4 steps of 16 lanes: dpad = 64*T
    const int dpad = T * 64;
    float* qs = reinterpret_cast<float*>(smem);             // [NQ][dpad]
    float* ls = qs + NQ * dpad;                             // [NQ][k] keys, best first
    uint32_t* li = reinterpret_cast<uint32_t*>(ls + NQ * k);
    int* lock = reinterpret_cast<int*>(li + NQ * k);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rsub = lane >> 4;
    if (tid < NQ) lock[tid] = 0;
    for (int i = tid; i < NQ * dpad; i += 256) {
        const int j = i / dpad;
        qs[i] = j < nq_real ? qpad[i] : 0.f;
    }
    for (int i = tid; i < NQ * k; i += 256) {
        ls[i] = -INFINITY;
        li[i] = kInvalidRow;
    }
    __syncthreads();

    const float4* qs4 = reinterpret_cast<const float4*>(qs);
    const int64_t ngroups = (ntotal + 3) >> 2;
    const int64_t g_begin = (int64_t)blockIdx.x * groups_per_block;
    const int64_t g_end = min(g_begin + groups_per_block, ngroups);
    // the sign of the prior term: f = s + weight * p (inner product), f = dist - weight * p (L2)
    const float wsgn = METRIC == CSS_METRIC_IP ? weight : -weight;

    float gcache[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) gcache[j] = -INFINITY;
    int iter = 0;

    for (int64_t g = g_begin + wave; g < g_end; g += kWaves, ++iter) {
        // (k_scan_small: the thresholds refreshed at the top, so that the FMA block and its consumers stay one basic block)
        if ((iter & 15) == 0) {
#pragma unroll
            for (int j = 0; j < NQ; ++j)
                gcache[j] = key2f(__hip_atomic_load(&gthr[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }

        const int64_t row = g * 4 + rsub;
        const bool in_range = row < ntotal;
        const int64_t rowc = in_range ? row : ntotal - 1;
        const bool valid = in_range && (mask == nullptr || ((mask[rowc >> 5] >> (rowc & 31)) & 1u));
        const float4* xr = xb + rowc * (int64_t)(T * 16) + sub;
        // once per row (the 16 lanes of a row read one word), unconditionally: a branch on the pointer, or the other
        // index width, costs 10 to 20 VGPRs in the NQ = 1 kernels (DESIGN.md 3.2g has the table)
        float pr = 0.f;
        if constexpr (HASP) pr = METRIC == CSS_METRIC_IP ? prior[rowc] : prior[(uint32_t)rowc];

        float acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] = 0.f;
        // NQ > 1: query fragments stay in LDS (k_scan_small: pinning them in VGPRs costs all the occupancy)
        if constexpr (NQ > 1) asm volatile("" ::: "memory");

        if constexpr (TT > 0) {
            float4 xv[TT > 0 ? TT : 1];
#pragma unroll
            for (int t = 0; t < TT; ++t) xv[t] = scan_row_load(xr + t * 16);
#pragma unroll
            for (int t = 0; t < TT; ++t) {
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const float4 q = qs4[j * (TT * 16) + t * 16 + sub];
                    if constexpr (METRIC == CSS_METRIC_IP) {
                        acc[j] = fmaf(xv[t].x, q.x, acc[j]);
                        acc[j] = fmaf(xv[t].y, q.y, acc[j]);
                        acc[j] = fmaf(xv[t].z, q.z, acc[j]);
                        acc[j] = fmaf(xv[t].w, q.w, acc[j]);
                    } else {
                        float dx = xv[t].x - q.x, dy = xv[t].y - q.y, dz = xv[t].z - q.z, dw = xv[t].w - q.w;
                        acc[j] = fmaf(dx, dx, acc[j]);
                        acc[j] = fmaf(dy, dy, acc[j]);
                        acc[j] = fmaf(dz, dz, acc[j]);
                        acc[j] = fmaf(dw, dw, acc[j]);
                    }
                }
                if constexpr (NQ > 1) __builtin_amdgcn_sched_barrier(0);   // (k_scan_small: keeps the LDS reads per column step)
            }
        } else {
            for (int t = 0; t < T; ++t) {
                const float4 x = scan_row_load(xr + t * 16);
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const float4 q = qs4[j * (T * 16) + t * 16 + sub];
                    if constexpr (METRIC == CSS_METRIC_IP) {
                        acc[j] = fmaf(x.x, q.x, acc[j]);
                        acc[j] = fmaf(x.y, q.y, acc[j]);
                        acc[j] = fmaf(x.z, q.z, acc[j]);
                        acc[j] = fmaf(x.w, q.w, acc[j]);
                    } else {
                        float dx = x.x - q.x, dy = x.y - q.y, dz = x.z - q.z, dw = x.w - q.w;
                        acc[j] = fmaf(dx, dx, acc[j]);
                        acc[j] = fmaf(dy, dy, acc[j]);
                        acc[j] = fmaf(dz, dz, acc[j]);
                        acc[j] = fmaf(dw, dw, acc[j]);
                    }
                }
            }
        }

        // every key and pass flag in this basic block, one combined ballot (k_scan_small)
        float sc[NQ];
        bool anyp = false;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float s = fmaf(wsgn, pr, row16_allsum(acc[j]));   // THE change: the fused value is the key
            if constexpr (METRIC == CSS_METRIC_L2) s = -s;
            sc[j] = s;
            const float lthr = ls[j * k + (k - 1)];
            // non-strict: an equal key with a lower row id must still reach the comparator
            anyp |= (s >= lthr) & (s >= gcache[j]) & (j < nq_real);  // '&': no short-circuit branches
        }
        if (__ballot(anyp && valid && sub == 0) == 0ull) continue;

        for (int j = 0; j < nq_real; ++j) {
            float s = sc[0];
#pragma unroll
            for (int u = 1; u < NQ; ++u) s = j == u ? sc[u] : s;
            const float lthr = ls[j * k + (k - 1)];
            const float gj = key2f(__hip_atomic_load(&gthr[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const bool pass = valid && sub == 0 && s >= lthr && s >= gj;
            unsigned long long m = __ballot(pass);
            if (m == 0ull) continue;
            // slow path: serialise on the block-shared list of query j
            if (lane == 0) {
                while (atomicCAS(&lock[j], 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            bool changed = false;
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const float cs = __shfl(s, l);
                const uint32_t cid = (uint32_t)(g * 4 + (l >> 4));
                changed |= wave_insert<uint32_t>(ls + j * k, li + j * k, k, cs, cid, lane);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            const float kth = ls[j * k + (k - 1)];
            if (lane == 0) {
                atomicExch(&lock[j], 0);
                if (changed && kth > gj) atomicMax(&gthr[j], f2key(kth));
            }
        }
    }
    __syncthreads();
    // part layout: [q][block][k]
    const int G = gridDim.x;
    for (int i = tid; i < nq_real * k; i += 256) {
        const int j = i / k, p = i - j * k;
        const size_t o = ((size_t)j * G + blockIdx.x) * k + p;
        part_s[o] = ls[i];
        part_i[o] = li[i];
    }
}

// The raw scores of the n = nq * k returned rows, behind the merge: 16 lanes per result entry (4 entries per wave, 16
// per block), the sweep's own chain over the row (see the head of this file).  I: global ids, -1 = a padded slot,
// which gets `pad`.  qpad: the prepared queries [nq][dpad]; xb is not read for padded slots (an empty index passes null).
template <int METRIC>
__global__ __launch_bounds__(256) void k_prior_scores(const float4* __restrict__ xb, const float* __restrict__ qpad,
                                                      const int64_t* __restrict__ I, int64_t n, int k, int T,
                                                      int64_t id_base, float pad, float* __restrict__ S) {
    const int sub = threadIdx.x & 15;
    const int64_t e = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int64_t ec = e < n ? e : n - 1;   // (whole 16-lane rows take part in the DPP reduction)
    const int64_t id = I[ec];
    float acc = 0.f;
    if (id >= 0) {
        const float4* xr = xb + (id - id_base) * (int64_t)(T * 16) + sub;
        const float4* qr = reinterpret_cast<const float4*>(qpad) + (ec / k) * (int64_t)(T * 16) + sub;
        for (int t = 0; t < T; ++t) {
            const float4 x = xr[t * 16], q = qr[t * 16];
            if constexpr (METRIC == CSS_METRIC_IP) {
                acc = fmaf(x.x, q.x, acc);
                acc = fmaf(x.y, q.y, acc);
                acc = fmaf(x.z, q.z, acc);
                acc = fmaf(x.w, q.w, acc);
            } else {
                float dx = x.x - q.x, dy = x.y - q.y, dz = x.z - q.z, dw = x.w - q.w;
                acc = fmaf(dx, dx, acc);
                acc = fmaf(dy, dy, acc);
                acc = fmaf(dz, dz, acc);
                acc = fmaf(dw, dw, acc);
            }
        }
    }
    const float s = row16_allsum(acc);
    if (e < n && sub == 0) S[e] = id >= 0 ? s : pad;
}
