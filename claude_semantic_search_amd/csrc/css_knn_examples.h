// css_knn_examples.h -- search by examples on the flat index: the k best rows under
//     best positive score - gamma * best negative score
// for a SET of example vectors ("more like these, and not like that one"; "anything that matches any of these
// phrasings").  Included by css_index.hip (inside its anonymous namespace, after k_scan_small: it reuses scan_row_load
// and kWaves, and row16_allsum / wave_insert / f2key of css_knn_kernels.h).
//
// Vector stores call this recommend, more-like-these or positive / negative examples.  It cannot be assembled from
// the other searches: a row's value under the negatives can sit anywhere below an over-fetched list, and a maximum
// of scores is not the score of some combined vector.  So the fused value is the key of the sweep itself.
//
// One request has m = npos + nneg <= 16 examples, as an example table [m][dpad] (positives first).  With s_j the score
// of a row against example j (the sweep's own fp32 chain: the inner product, or the squared L2 distance):
//     inner product   P = max_{j < npos} s_j, N = max_{npos <= j < m} s_j   larger is better, key = f
//     squared L2      P = min_{j < npos} s_j, N = min_{npos <= j < m} s_j   smaller is better, key = -f (f may be < 0)
//     f = P when there is no negative, else f = fmaf(-gamma, N, P)
// Maxima and minima are exact, so f is one rounding away from the scores of the exact fp32 search.
//
// k_scan_examples is the non-FIX sweep of k_scan_small with the example table where the queries sit and ONE change:
// behind row16_allsum the NQ scores of a row collapse to ONE key, which goes into ONE list -- one ls / li of k entries,
// one lock, one gthr word, part lists [block][k].  Everything else is k_scan_small's: thread layout (block = 4 waves, a
// wave instruction covers 4 rows, 16 lanes x float4 per row and column step), one fp32 fmaf chain per lane and example
// over the padded row, DPP row reduction, non-temporal row loads, the mask bit per row, wave_insert, the grid-wide
// threshold.  Keys are "larger is better" for both metrics, so k_merge_final<METRIC> (one "query"), sweep_grid and
// grow_part serve unchanged, as for k_scan_prior.  NQ is the smallest of 1 / 2 / 8 / 16 that holds m; a padded slot
// j >= m takes part in neither extremum (a zero example scores 0 under the inner product and ||x||^2 under L2, and
// either can win when the real scores lie on the other side).
//
// Excluded rows (the examples given as stored rows, where the caller wants them left out) are at most 16 local row
// numbers in LDS.  They are tested only on the slow path, in `pass`, before wave_insert: an excluded row is a near-best
// row by construction, so it reaches the slow path anyway, and the fast path pays nothing.
//
// The sweep body (row addressing, mask test, fmaf blocks) now exists FIVE times on purpose: k_scan_small,
// k_range_small, k_scan_prior, here and k_facet_small (css_knn_facets.h); css_knn_range.h and
// profiles/flat_index_refactor_shared_sweep_attempts.txt say why it is not one function.  A change to one is made to
// all five.
//
// The raw score.  The call also returns S = P, the best positive score of a returned row, so that similarity
// thresholds keep their meaning.  As in css_knn_prior.h it is not carried through the lists: k_example_scores runs ONCE
// behind the merge and re-forms the scores of the k returned rows against the positives with the very chain of the
// sweep (lane `sub` of a 16-lane row walks columns 64 t + 4 sub, t ascending, x y z w, then row16_allsum): the same
// operations in the same order on the same operands, hence the same bits -- D == S without negatives, and
// D == fmaf(-gamma, N, S) with them.
#pragma once

constexpr int kMaxExamples = CSS_MAX_EXAMPLES;

template <int NQ, int TT, int METRIC>
__global__ __launch_bounds__(256, 4) void k_scan_examples(const float4* __restrict__ xb, const float* __restrict__ epad,
                                                          int64_t ntotal, int T_rt, int k, int64_t groups_per_block,
                                                          int* __restrict__ gthr, float* __restrict__ part_s,
                                                          uint32_t* __restrict__ part_i, int npos, int m, float gamma,
                                                          const uint32_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ excl, int nexcl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = TT > 0 ? TT : T_rt;  // float4 steps of 16 lanes: dpad = 64*T
    const int dpad = T * 64;
    float* qs = reinterpret_cast<float*>(smem);             // [NQ][dpad] the example table
    float* ls = qs + NQ * dpad;                             // [k] keys, best first
    uint32_t* li = reinterpret_cast<uint32_t*>(ls + k);     // [k]
    int* lock = reinterpret_cast<int*>(li + k);             // [2] (one lock, one word of padding)
    uint32_t* ex = reinterpret_cast<uint32_t*>(lock + 2);   // [kMaxExamples] excluded local rows

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rsub = lane >> 4;
    if (tid == 0) lock[0] = 0;
    if (tid < kMaxExamples) ex[tid] = tid < nexcl ? excl[tid] : kInvalidRow;
    for (int i = tid; i < NQ * dpad; i += 256) {
        const int j = i / dpad;
        qs[i] = j < m ? epad[i] : 0.f;
    }
    for (int i = tid; i < k; i += 256) {
        ls[i] = -INFINITY;
        li[i] = kInvalidRow;
    }
    __syncthreads();

    const float4* qs4 = reinterpret_cast<const float4*>(qs);
    const int64_t ngroups = (ntotal + 3) >> 2;
    const int64_t g_begin = (int64_t)blockIdx.x * groups_per_block;
    const int64_t g_end = min(g_begin + groups_per_block, ngroups);
    const bool has_neg = m > npos;
    // The slow path below is written as k_scan_small writes it: a loop over the lists with a trip count the compiler
    // does not know, every access indexed by the list.  There is ONE list; the count is made opaque here.  Written as
    // a plain block the compiler merges the slow path's LDS reads with those of the sweep and the <1, 12, *> and
    // <2, *, *> kernels lose one to three waves per SIMD against their siblings (DESIGN.md 3.2h has the table).
    int nlists = 1;
    asm volatile("" : "+s"(nlists));
    const float ngamma = -gamma;

    float gcache = -INFINITY;
    int iter = 0;

    for (int64_t g = g_begin + wave; g < g_end; g += kWaves, ++iter) {
        // (k_scan_small: the threshold refreshed at the top, so that the FMA block and its consumers stay one basic block)
        if ((iter & 15) == 0) gcache = key2f(__hip_atomic_load(gthr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));

        const int64_t row = g * 4 + rsub;
        const bool in_range = row < ntotal;
        const int64_t rowc = in_range ? row : ntotal - 1;
        const bool valid = in_range && (mask == nullptr || ((mask[rowc >> 5] >> (rowc & 31)) & 1u));
        const float4* xr = xb + rowc * (int64_t)(T * 16) + sub;

        float acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] = 0.f;
        // NQ > 1: example fragments stay in LDS (k_scan_small: pinning them in VGPRs costs all the occupancy)
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

        // THE change: the NQ scores of the row collapse to one key, in the basic block of the chains (k_scan_small).
        // A slot j >= m is padding and enters neither extremum; the selects are on wave-uniform conditions.
        float key;
        if constexpr (NQ == 1) {
            key = row16_allsum(acc[0]);   // (m == npos == 1: the one positive's score)
        } else {
            float P = METRIC == CSS_METRIC_IP ? -INFINITY : INFINITY, N = P;
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const float s = row16_allsum(acc[j]);
                const float e = METRIC == CSS_METRIC_IP ? fmaxf(P, s) : fminf(P, s);
                const float en = METRIC == CSS_METRIC_IP ? fmaxf(N, s) : fminf(N, s);
                P = j < npos ? e : P;
                N = ((j >= npos) & (j < m)) ? en : N;
            }
            key = has_neg ? fmaf(ngamma, N, P) : P;   // (no negative: N is infinite, and f is P itself)
        }
        if constexpr (METRIC == CSS_METRIC_L2) key = -key;
        const float lthr0 = ls[k - 1];
        // non-strict: an equal key with a lower row id must still reach the comparator
        const bool anyp = (key >= lthr0) & (key >= gcache);
        if (__ballot(anyp && valid && sub == 0) == 0ull) continue;

        for (int jj = 0; jj < nlists; ++jj) {
            const float lthr = ls[jj * k + (k - 1)];
            const float gj = key2f(__hip_atomic_load(&gthr[jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const bool pass = valid && sub == 0 && key >= lthr && key >= gj;
            unsigned long long mm = __ballot(pass);
            // slow path only: the rows the caller excluded leave `pass` (scalar code: an excluded row of this group
            // is row d of its 4, whose flag is that of lane 16 d)
            for (int u = 0; u < nexcl; ++u) {
                const uint32_t d = ex[u] - (uint32_t)(g * 4);
                if (d < 4u) mm &= ~(1ull << (d * 16));
            }
            if (mm == 0ull) continue;
            // serialise on the block-shared list
            if (lane == 0) {
                while (atomicCAS(&lock[jj], 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            bool changed = false;
            while (mm) {
                const int l = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const float cs = __shfl(key, l);
                const uint32_t cid = (uint32_t)(g * 4 + (l >> 4));
                changed |= wave_insert<uint32_t>(ls + jj * k, li + jj * k, k, cs, cid, lane);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            const float kth = ls[jj * k + (k - 1)];
            if (lane == 0) {
                atomicExch(&lock[jj], 0);
                if (changed && kth > gj) atomicMax(&gthr[jj], f2key(kth));
            }
        }
    }
    __syncthreads();
    // part layout: [block][k]
    for (int i = tid; i < k; i += 256) {
        const size_t o = (size_t)blockIdx.x * k + i;
        part_s[o] = ls[i];
        part_i[o] = li[i];
    }
}

// S = P of the k returned rows, behind the merge: one block per returned row, 16 lanes per (row, positive example), the
// sweep's own chain over the row (see the head of this file); the negatives are not needed for S.  I: global ids,
// -1 = a padded slot, which gets `pad` (xb is not read for it: an empty index passes null).  The loads of four column
// steps are issued ahead of their chain: the dependent load-then-fmaf loop of k_prior_scores costs 24 us on 768
// columns.
template <int METRIC>
__global__ __launch_bounds__(256) void k_example_scores(const float4* __restrict__ xb, const float* __restrict__ epad,
                                                        const int64_t* __restrict__ I, int npos, int T, int64_t id_base,
                                                        float pad, float* __restrict__ S) {
    __shared__ float sp[kMaxExamples];
    const int sub = threadIdx.x & 15, j = threadIdx.x >> 4;   // j: the example of this 16-lane row
    const int64_t id = I[blockIdx.x];
    if (id < 0) {   // (block-uniform)
        if (threadIdx.x == 0) S[blockIdx.x] = pad;
        return;
    }
    float acc = 0.f;
    if (j < npos) {
        const float4* xr = xb + (id - id_base) * (int64_t)(T * 16) + sub;
        const float4* qr = reinterpret_cast<const float4*>(epad) + j * (int64_t)(T * 16) + sub;
        for (int t0 = 0; t0 < T; t0 += 4) {
            float4 x[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = min(t0 + u, T - 1);   // (a step beyond the row re-reads the last one and is not summed)
                x[u] = xr[t * 16];
                q[u] = qr[t * 16];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + u >= T) break;
                if constexpr (METRIC == CSS_METRIC_IP) {
                    acc = fmaf(x[u].x, q[u].x, acc);
                    acc = fmaf(x[u].y, q[u].y, acc);
                    acc = fmaf(x[u].z, q[u].z, acc);
                    acc = fmaf(x[u].w, q[u].w, acc);
                } else {
                    float dx = x[u].x - q[u].x, dy = x[u].y - q[u].y, dz = x[u].z - q[u].z, dw = x[u].w - q[u].w;
                    acc = fmaf(dx, dx, acc);
                    acc = fmaf(dy, dy, acc);
                    acc = fmaf(dz, dz, acc);
                    acc = fmaf(dw, dw, acc);
                }
            }
        }
    }
    const float s = row16_allsum(acc);   // (whole 16-lane rows take part in the DPP reduction)
    if (sub == 0) sp[j] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float P = sp[0];
        for (int u = 1; u < npos; ++u) P = METRIC == CSS_METRIC_IP ? fmaxf(P, sp[u]) : fminf(P, sp[u]);
        S[blockIdx.x] = P;
    }
}
