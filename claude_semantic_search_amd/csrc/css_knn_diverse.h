// css_knn_diverse.h -- diversified search on the flat index: maximal marginal relevance (MMR) over a pool of the best rows.
// Included by css_index.hip (inside its anonymous namespace, after css_knn_group.h).
//
// A diversified search is the ordinary ranked, masked search for a pool of m <= 128 rows followed by a greedy
// selection of k of them: pick 0 is the pool's best row, and every further pick is the unpicked candidate c with the
// largest  v_c = lam * rel_c - (1 - lam) * max_{picked p} sim(c, p)  (include/css_hip.h has the definition).  The scan
// kernels stay untouched; what is new reads (k - 1) * m stored rows per query:
//
//   k_mmr_select   one 256-thread block per query.  The penalty max_p sim(c, p) is kept per candidate in LDS and a step
//                  updates it against the LAST pick only, so k - 1 columns of the pool's Gram matrix are formed, never
//                  the matrix.  A wave takes every fourth candidate, four of them at a time; its lanes stride the fp32 rows
//                  where they lie (rows.xb + slot * dpad: no gathered copy) and a DPP reduction closes each sum.  A block-wide argmax
//                  (score, then the smaller list position) ends the step.
#pragma once

// Ds / Is: [nq, m] best-first lists of the pool search (ids global, pads -1 at the tail).  D / I: [nq, k] picks in
// pick order, padded behind min(k, valid candidates).  n rows at xb, dpad floats apart; m <= CSS_KERNEL_MAX_K.
// The set of picked candidates is a 128-bit mask that every thread keeps in (wave-uniform) registers: each thread
// closes the argmax from the same four LDS words, so no flag has to cross a barrier.  All barriers sit in loops whose
// bounds are the same for the whole block (one query per block: its valid count mv is block-uniform) and no thread
// returns in front of one.  Rows are read only through a slot checked against n, whatever the lists hold.
// one term of a similarity sum: a product (inner product) or a squared difference (L2: copies of a row give exactly 0)
template <int METRIC>
__device__ __forceinline__ float mmr_term(float x, float y, float acc) {
    if (METRIC == CSS_METRIC_IP) return fmaf(x, y, acc);
    const float dlt = x - y;
    return fmaf(dlt, dlt, acc);
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_mmr_select(const float* __restrict__ Ds, const int64_t* __restrict__ Is,
                                                    const float* __restrict__ xb, int64_t n, int64_t id_base, int dim,
                                                    int dpad, int m, int k, float lam, float pad, float* __restrict__ D,
                                                    int64_t* __restrict__ I) {
    __shared__ float rel[CSS_KERNEL_MAX_K];
    __shared__ float pen[CSS_KERNEL_MAX_K];
    __shared__ uint32_t slot[CSS_KERNEL_MAX_K];   // row of the candidate (id - id_base), kInvalidRow: a pad
    __shared__ float red_v[4];
    __shared__ int red_c[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t j = blockIdx.x;
    const float* Dj = Ds + (size_t)j * m;
    const int64_t* Ij = Is + (size_t)j * m;
    float* Do = D + (size_t)j * k;
    int64_t* Io = I + (size_t)j * k;
    const bool reads = lam != 1.0f;   // lam == 1: v = rel whatever the rows hold, so they are not read
    const float oml = 1.0f - lam;
    bool valid = false;
    if (tid < CSS_KERNEL_MAX_K) {
        float s = pad;
        uint32_t r = kInvalidRow;
        if (tid < m) {
            const int64_t id = Ij[tid];
            const uint64_t u = (uint64_t)id - (uint64_t)id_base;   // (unsigned: an id below id_base wraps beyond n)
            valid = id >= 0 && u < (uint64_t)n;
            if (valid) {
                s = Dj[tid];
                r = (uint32_t)u;
            }
        }
        rel[tid] = METRIC == CSS_METRIC_IP ? s : -s;
        pen[tid] = reads ? -INFINITY : 0.f;   // max over no picks; without row reads the term is 0 * 0
        slot[tid] = r;
    }
    const int mv = __syncthreads_count(valid);   // valid candidates: the front of the list
    int np = slot[0] != kInvalidRow ? min(k, mv) : 0;   // picks to make
    unsigned long long tk0 = 0ull, tk1 = 0ull;   // picked candidates 0..63 / 64..127
    int last = 0;
    if (np > 0) {
        tk0 = 1ull;
        if (tid == 0) {
            Do[0] = Dj[0];
            Io[0] = Ij[0];
        }
    }
    for (int t = 1; t < np; ++t) {
        if (reads) {   // pen_c = max(pen_c, sim(c, last)) for every candidate still to be had
            const float* a = xb + (size_t)slot[last] * dpad;
            // four candidates of the wave at a time: their row loads are in flight together and share the loads of
            // the last pick's row.  A candidate that is a pad or picked already reads the last pick's row instead
            // (valid memory, result unused); the summation order of a candidate does not depend on its neighbours
            for (int c0 = wave; c0 < m; c0 += 16) {
                bool on[4];
                const float* b[4];
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                bool any = false;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + 4 * u;
                    on[u] = c < m && slot[min(c, CSS_KERNEL_MAX_K - 1)] != kInvalidRow &&
                            ((c < 64 ? tk0 >> c : tk1 >> (c - 64)) & 1ull) == 0ull;
                    b[u] = on[u] ? xb + (size_t)slot[c] * dpad : a;
                    any = any || on[u];
                }
                if (!any) continue;   // (wave-uniform)
                if ((dim & 3) == 0) {   // (rows start on 16-byte boundaries)
                    for (int e = lane; e < dim / 4; e += 64) {
                        const float4 x = reinterpret_cast<const float4*>(a)[e];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const float4 y = reinterpret_cast<const float4*>(b[u])[e];
                            acc[u] = mmr_term<METRIC>(x.x, y.x, acc[u]);
                            acc[u] = mmr_term<METRIC>(x.y, y.y, acc[u]);
                            acc[u] = mmr_term<METRIC>(x.z, y.z, acc[u]);
                            acc[u] = mmr_term<METRIC>(x.w, y.w, acc[u]);
                        }
                    }
                } else {
                    for (int e = lane; e < dim; e += 64) {
                        const float x = a[e];
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[u] = mmr_term<METRIC>(x, b[u][e], acc[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float sum = wave_allsum(acc[u]);
                    const float sim = METRIC == CSS_METRIC_IP ? sum : -sum;
                    if (on[u] && lane == 0) pen[c0 + 4 * u] = fmaxf(pen[c0 + 4 * u], sim);
                }
            }
        }
        __syncthreads();
        // argmax of v over the unpicked valid candidates, ties to the smaller c; a NaN counts as -inf, and 128 is the
        // position of "none" (any candidate beats it on the tie rule)
        float bv = -INFINITY;
        int bc = CSS_KERNEL_MAX_K;
        if (valid && ((tid < 64 ? tk0 >> tid : tk1 >> (tid - 64)) & 1ull) == 0ull) {
            const float v = __fsub_rn(__fmul_rn(lam, rel[tid]), __fmul_rn(oml, pen[tid]));   // (no contraction: three roundings)
            bv = v > -INFINITY ? v : -INFINITY;
            bc = tid;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oc = __shfl_xor(bc, o);
            if (ov > bv || (ov == bv && oc < bc)) {
                bv = ov;
                bc = oc;
            }
        }
        if (lane == 0) {
            red_v[wave] = bv;
            red_c[wave] = bc;
        }
        __syncthreads();
        bv = red_v[0];
        bc = red_c[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = red_v[w];
            const int oc = red_c[w];
            if (ov > bv || (ov == bv && oc < bc)) {
                bv = ov;
                bc = oc;
            }
        }
        if (bc >= m) {   // none left (t < mv rules it out for the lists of a search); the same in every thread
            np = t;
            break;
        }
        if (bc < 64) tk0 |= 1ull << bc;
        else tk1 |= 1ull << (bc - 64);
        last = bc;
        if (tid == 0) {
            Do[t] = Dj[bc];
            Io[t] = Ij[bc];
        }
    }
    for (int t = np + tid; t < k; t += 256) {
        Do[t] = pad;
        Io[t] = -1;
    }
}
