// css_knn_facets.h -- facet counts on the flat index: per query, how many rows within a radius fall into each bucket
// of a per-row int32 column, and the best such row of every bucket.  Included by css_index.hip (inside its anonymous
// namespace, after css_knn_range.h: it reuses scan_row_load and kWaves, and row16_allsum of css_knn_kernels.h).
//
// This is the `terms` / `date_histogram` aggregation of Elasticsearch, Qdrant's facet API, Vespa's grouping: the
// answer is nq * nbuckets integers whatever the number of hits, so nothing is appended, nothing is swept twice and
// nothing is sorted.  A row hits query j when score > radius (inner product) or dist < radius (squared L2), STRICT,
// NaN never: the predicate of k_range_small on the same float.
//
// k_facet_small is the sweep of k_range_small with the append replaced by a table: same thread layout (block = 4
// waves, a wave instruction covers 4 rows, 16 lanes x float4 per row and column step, queries in LDS, DPP row
// reduction, non-temporal row loads, mask bit tested per row) and the SAME fp32 fmaf chain per lane, so a row hits
// here exactly when it hits in css_index_range_search on the same index and radius, with the same score.  The sweep
// body is the FIFTH copy (css_knn_range.h says why it is not shared): a change to one is made to all five.
//
// Table.  Entry (j, b) of the sweep's table is a uint32 count and a uint64 key, both only ever touched by integer
// atomics (add, max).  key = [order-preserving image of the fp32 score, inverted for L2 | ~row], so the largest key is
// the best score and, among equal scores, the smallest row; 0 means "no hit" (the image of a score that can hit is
// never 0: only NaN patterns map there).  Integer add and max commute, so the table does not depend on the order in
// which the waves arrive: the result is the same bytes on every run.  A hit whose bucket is outside [0, nbuckets)
// (negative label, label beyond the caller's range, or no column at all) is counted in unbucketed[j] only; total[j]
// counts every hit.  total and unbucketed are kept per WAVE in uniform registers (popcount of the hit ballot) and
// added to the global words once, when the wave leaves: no atomic of theirs is inside the row loop.
//
// Placement of the table, chosen by the host per sweep (facet_lds_fits in css_index.hip has the limit):
//   LDS_TABLE = true   [nq_real][nbuckets] keys then counts in LDS behind the query rows, zeroed at block start,
//                      updated with LDS atomics by the row's head lane, and every non-zero entry flushed at block end
//                      with ONE global atomicAdd and ONE global 64-bit atomicMax (agent scope, relaxed).  Few buckets
//                      and many hits: direct global atomics would all land on a handful of addresses.
//   LDS_TABLE = false  hits update the global table directly; a relaxed load of the key first skips the 64-bit max
//                      when the entry already holds a key at least as large (the entry only grows, so a stale value
//                      costs a redundant atomic, never a wrong result).
#pragma once

// [order-preserving image of s (larger = better) | ~row]
template <int METRIC>
__device__ __forceinline__ unsigned long long facet_key(float s, uint32_t row) {
    uint32_t u = __float_as_uint(s + 0.f);   // (-0 and +0 are one score)
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if constexpr (METRIC != CSS_METRIC_IP) u = ~u;
    return ((unsigned long long)u << 32) | (unsigned long long)(uint32_t)~row;
}

template <int NQ, int TT, int METRIC, bool LDS_TABLE>
__global__ __launch_bounds__(256, 4) void k_facet_small(const float4* __restrict__ xb, const float* __restrict__ qpad,
                                                        int64_t ntotal, int T_rt, int64_t groups_per_block, int nq_real,
                                                        const uint32_t* __restrict__ mask, float radius,
                                                        const int32_t* __restrict__ bucket, int nbuckets,
                                                        unsigned int* __restrict__ totals /* [16] total | [16] unbucketed */,
                                                        unsigned int* __restrict__ cnt /* [nq_real][nbuckets] */,
                                                        unsigned long long* __restrict__ best /* [nq_real][nbuckets] */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = TT > 0 ? TT : T_rt;  // float4 steps of 16 lanes: dpad = 64*T
    const int dpad = T * 64;
    float* qs = reinterpret_cast<float*>(smem);   // [NQ][dpad]
    const int nent = nq_real * nbuckets;          // (LDS_TABLE: the host checked that the table fits)
    unsigned long long* best_l = reinterpret_cast<unsigned long long*>(smem + (size_t)NQ * dpad * 4);   // [nent]
    unsigned int* cnt_l = reinterpret_cast<unsigned int*>(best_l + (LDS_TABLE ? nent : 0));             // [nent]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rsub = lane >> 4;
    for (int i = tid; i < NQ * dpad; i += 256) {
        const int j = i / dpad;
        qs[i] = j < nq_real ? qpad[i] : 0.f;
    }
    if constexpr (LDS_TABLE) {
        for (int i = tid; i < nent; i += 256) {
            best_l[i] = 0ull;
            cnt_l[i] = 0u;
        }
    }
    __syncthreads();

    const float4* qs4 = reinterpret_cast<const float4*>(qs);
    const int64_t ngroups = (ntotal + 3) >> 2;
    const int64_t g_begin = (int64_t)blockIdx.x * groups_per_block;
    const int64_t g_end = min(g_begin + groups_per_block, ngroups);

    unsigned int tot[NQ], unb[NQ];   // wave-uniform: hits / unbucketed hits of this wave so far
#pragma unroll
    for (int j = 0; j < NQ; ++j) tot[j] = unb[j] = 0u;

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
        const bool rowhit = anyh && head;
        if (__ballot(rowhit) == 0ull) continue;

        // the bucket of a row that hit some query (head => the row exists); anything outside [0, nbuckets) is -1
        int b = -1;
        if (rowhit && bucket != nullptr) {
            const int v = bucket[row];
            b = (unsigned int)v < (unsigned int)nbuckets ? v : -1;
        }

#pragma unroll
        for (int j = 0; j < NQ; ++j) {   // (no break / continue: the loop must unroll, sc[] stays in registers)
            const float s = sc[j];
            const bool hit = head && j < nq_real && (METRIC == CSS_METRIC_IP ? s > radius : s < radius);
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) {
                tot[j] += (unsigned int)__popcll(m);
                unb[j] += (unsigned int)__popcll(__ballot(hit && b < 0));
                if (hit && b >= 0) {
                    const unsigned long long key = facet_key<METRIC>(s, (uint32_t)row);
                    const int e = j * nbuckets + b;
                    if constexpr (LDS_TABLE) {
                        __hip_atomic_fetch_add(cnt_l + e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_max(best_l + e, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        __hip_atomic_fetch_add(cnt + e, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (__hip_atomic_load(best + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key)
                            __hip_atomic_fetch_max(best + e, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        }
    }

    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (tot[j]) __hip_atomic_fetch_add(totals + j, tot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (unb[j]) __hip_atomic_fetch_add(totals + 16 + j, unb[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (LDS_TABLE) {
        __syncthreads();
        for (int i = tid; i < nent; i += 256) {
            const unsigned int c = cnt_l[i];
            if (c) {   // (a counted entry has a key)
                __hip_atomic_fetch_add(cnt + i, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_max(best + i, best_l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
