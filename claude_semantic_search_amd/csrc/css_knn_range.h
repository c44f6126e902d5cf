// css_knn_range.h -- range search on the flat index: every row within a radius, as a variable-length hit list.
// Included by css_index.hip (inside its anonymous namespace, after k_scan_small: it reuses scan_row_load and kWaves,
// and row16_allsum of css_knn_kernels.h).
//
// faiss has this as IndexFlat::range_search(x, radius).  A row hits query j when score > radius (inner product) or
// dist < radius (squared L2): STRICT, the comparison of faiss' RangeSearchBlockResultHandler [from knowledge of the
// public faiss sources; faiss is not installed here, so that was not checked against a running faiss].
//
// k_range_small is the sweep of k_scan_small without its lists: same thread layout (block = 4 waves, a wave
// instruction covers 4 rows, 16 lanes x float4 per row and column step, queries in LDS, DPP row reduction,
// non-temporal row loads, mask bit tested per row), same arithmetic (one fp32 fmaf chain per lane over the padded
// row, IP = dot, L2 = sum of squared differences, which cannot go negative).  It reads the fp32 rows only, so the
// answer does not depend on which reduced-precision copies the index keeps.  The fp32 score the kernel formed is the
// value compared with the radius AND the value returned.  The sweep body (row addressing, mask test, fmaf blocks) is
// kept FIVE times on purpose, here, in k_scan_small, in k_scan_prior (css_knn_prior.h), in k_scan_examples
// (css_knn_examples.h) and in k_facet_small (css_knn_facets.h): moved into one __forceinline__ function it changed the
// register allocation of the kernels that shared it (profiles/flat_index_refactor_shared_sweep_attempts.txt), so a
// change to one is made to all five.
//
// Appending.  Query slot j owns pool entries [j * cap, (j + 1) * cap) and the counter cnt[j].  Per wave instruction
// and query with at least one hit among the 4 rows: ballot, popcount, ONE returning agent-scope integer atomicAdd by
// lane 0 (never one per lane), lane rank = popcount of the lower hit lanes.  The counter keeps counting past `cap`
// and only the stores are skipped there, so a single sweep always yields the exact hit count of every query: when a
// pool was too small the host grows it to the counted size and sweeps ONCE more (css_index_range_search); no loop.
// The order of the entries of a query is whatever the waves' atomics made it; the host sorts every segment.
#pragma once

template <int NQ, int TT, int METRIC>
__global__ __launch_bounds__(256, 4) void k_range_small(const float4* __restrict__ xb, const float* __restrict__ qpad,
                                                        int64_t ntotal, int T_rt, int64_t groups_per_block, int nq_real,
                                                        const uint32_t* __restrict__ mask, float radius,
                                                        unsigned int* __restrict__ cnt, float* __restrict__ pool_s,
                                                        uint32_t* __restrict__ pool_i, unsigned int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = TT > 0 ? TT : T_rt;  // float4 steps of 16 lanes: dpad = 64*T
    const int dpad = T * 64;
    float* qs = reinterpret_cast<float*>(smem);   // [NQ][dpad]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rsub = lane >> 4;
    for (int i = tid; i < NQ * dpad; i += 256) {
        const int j = i / dpad;
        qs[i] = j < nq_real ? qpad[i] : 0.f;
    }
    __syncthreads();

    const float4* qs4 = reinterpret_cast<const float4*>(qs);
    const int64_t ngroups = (ntotal + 3) >> 2;
    const int64_t g_begin = (int64_t)blockIdx.x * groups_per_block;
    const int64_t g_end = min(g_begin + groups_per_block, ngroups);

    for (int64_t g = g_begin + wave; g < g_end; g += kWaves) {
        const int64_t row = g * 4 + rsub;
        const bool in_range = row < ntotal;
        const int64_t rowc = in_range ? row : ntotal - 1;
        const bool valid = in_range && (mask == nullptr || ((mask[rowc >> 5] >> (rowc & 31)) & 1u));
        const float4* xr = xb + rowc * (int64_t)(T * 16) + sub;

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

        // every score and hit flag in this basic block, one combined ballot: the usual row group hits nothing
        float sc[NQ];
        bool anyh = false;
        const bool head = valid && sub == 0;   // one lane per row reports it
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            sc[j] = row16_allsum(acc[j]);
            const bool h = METRIC == CSS_METRIC_IP ? sc[j] > radius : sc[j] < radius;   // NaN scores never hit
            anyh |= h & (j < nq_real);
        }
        if (__ballot(anyh && head) == 0ull) continue;

#pragma unroll
        for (int j = 0; j < NQ; ++j) {   // (no break / continue: the loop must unroll, sc[] stays in registers)
            const float s = sc[j];
            const bool hit = head && j < nq_real && (METRIC == CSS_METRIC_IP ? s > radius : s < radius);
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) {
                unsigned int base = 0;
                if (lane == 0) base = __hip_atomic_fetch_add(cnt + j, (unsigned int)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
                // 64-bit position: a counter below 2^32 plus a rank below 4, compared with cap without wrapping
                const uint64_t pos = (uint64_t)base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
                if (hit && pos < (uint64_t)cap) {
                    pool_s[(size_t)j * cap + pos] = s;
                    pool_i[(size_t)j * cap + pos] = (uint32_t)row;
                }
            }
        }
    }
}
