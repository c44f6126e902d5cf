// css_encoder.hip -- MPNet (all-mpnet-base-v2 architecture) and BERT (all-MiniLM-L6-v2, bge-*-en-v1.5) sentence
// encoders on gfx950.
//
// Replaces, behind include/css_hip.h, what the reference reaches through
// SentenceTransformer.encode() (src/embeddings.py:184-188, :216-222): MPNet
// encoder forward -> masked mean pooling -> L2 normalise.
// Tokenisation stays on the host (claude_semantic_search_amd/tokenizer.py); the
// boundary here is (packed input_ids, cu_seqlens).
//
// Pipeline per forward (one stream, no host syncs between kernels):
//   k_embed_ln -> 12 x [ k_gemm<QKV> -> attention -> k_gemm<RESID> -> k_layernorm
//                        -> k_gemm<GELU> -> k_gemm<RESID> -> k_layernorm ] -> k_pool_norm
// BERT is the same post-LN stack with absolute positions (+ token-type row 0, folded into the position table when the
// weights are finalised), no relative position bias, and mean or CLS pooling (css_encoder_cfg.arch / .pooling).
// css_encoder_forward_pairs (BERT cross-encoders) runs the same stack with a per-sequence segment start (type-1 tokens
// take `tdelta` in the embedding kernels), CLS rows without normalisation, then k_ce_head.
// css_encoder_forward_sparse (BERT masked-LM checkpoints) follows the stack with the head's transform (GEMM + GELU,
// k_mlm_ln), k_vocab_max (decoder GEMM with the maximum over each sequence's tokens in its epilogue) and k_vocab_topm.
// Residual stream / LayerNorm / softmax / pooling are fp32; GEMM and attention
// operands are bf16 (MFMA) in the product mode, fp32 in the verification mode.
#include "css_common.h"
#include "css_devbuf.h"
#include "css_encoder_kernels.h"
#include "../../include/css_synth.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace css;

namespace {

struct Param {
    float* p = nullptr;
    int64_t numel = 0;
    uint32_t synth_id = 0;
    float mean = 0.f, std = 0.02f;
    bool owned = true;     // false: a view into a fused tensor (q/k/v rows of the QKV weight / bias)
    bool synth = true;     // filled by css_encoder_init_synthetic (MPNet fills the fused tensor, BERT its q/k/v views)
    bool required = true;  // a checkpoint must name it (MPNet q/k/v views: the fused tensor or all three views)
};

struct LayerW {
    float *wqkv, *bqkv, *wo, *bo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
    bf16_t *wqkv_h, *wo_h, *w1_h, *w2_h;
    // LayerNorm-folded operands (k_fold_ln): the QKV weight carries gamma of the LayerNorm BEFORE this layer
    // (embedding LN / previous layer's output LN), the FFN1 weight gamma of this layer's attention LN
    bf16_t *wqkv_f = nullptr, *w1_f = nullptr;
    bf16_t *w2_p = nullptr, *wo_p = nullptr;   // W2 / Wo in bf16 with the K order of their blocked A operands (k_f32_to_bf16_kperm)
    float *dqkv = nullptr, *d1 = nullptr;   // d rows of the two folded GEMMs
    float *bo_f = nullptr, *b2_f = nullptr; // bias + beta of the LayerNorm whose output is the residual (EPI_RES)
};

__global__ void k_synth_fill(float* p, size_t n, uint64_t seed, float mean, float std) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = mean + std * css_synth_normal(seed, (uint64_t)i);
}

__global__ void k_build_bias_tab(const float* __restrict__ relw, const int* __restrict__ bucket, int heads, int maxL,
                                 float scale, float* __restrict__ tab) {
    const int n = 2 * maxL - 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * heads) return;
    const int h = i / n, r = i - h * n;
    tab[i] = scale * relw[bucket[r] * heads + h];  // bf16 path: log2(e) (scores in the log2 domain)
}

__global__ void k_zero_row(float* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

// BERT: out[p][c] = pemb[p][c] + row[c] (token-type row 0 folded into the position table)
__global__ void k_add_row(const float* __restrict__ pemb, const float* __restrict__ row, float* __restrict__ out, int rows,
                          int H) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * H) out[i] = pemb[i] + row[i % H];
}

// BERT: tdelta[c] = tte[1][c] - tte[0][c] (what a type-1 token adds on top of the folded position table)
__global__ void k_type_delta(const float* __restrict__ tte, float* __restrict__ out, int H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H) out[i] = tte[H + i] - tte[i];
}

}  // namespace

// Bucket of a relative position (rel = key - query), transformers'
// MPNetEncoder.relative_position_bucket (modeling_mpnet.py:312-348 in 5.15.0).
// Evaluated in double: the only integer-valued cases are |rel| = 16, 32, 64 where
// log(n/8)/log(16)*8 is exact in double as well (tests/test_encoder_host.py pins
// all 1023 values against the transformers implementation).
extern "C" int css_mpnet_rel_bucket(int rel, int num_buckets, int max_distance) {
    int n = -rel;
    const int half = num_buckets / 2;
    int ret = n < 0 ? half : 0;
    n = n < 0 ? -n : n;
    const int max_exact = half / 2;
    if (n < max_exact) return ret + n;
    const double v = std::log((double)n / max_exact) / std::log((double)max_distance / max_exact) * (half - max_exact);
    int large = max_exact + (int)v;
    if (large > half - 1) large = half - 1;
    return ret + large;
}

struct css_encoder {
    css_encoder_cfg cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    std::map<std::string, Param> params;
    float *wemb = nullptr, *pemb = nullptr, *embg = nullptr, *embb = nullptr, *relw = nullptr;
    float *tte = nullptr;        // BERT token_type_embeddings [2][H]
    float *pemb_eff = nullptr;   // position table the embedding kernels read: pemb (MPNet), pemb + tte[0] (BERT)
    float *tdelta = nullptr;     // BERT: tte[1] - tte[0] [H], added to the type-1 tokens of a pair batch
    std::vector<void*> extra;    // device buffers owned outside `params` (BERT fused QKV, pemb_eff)
    std::vector<LayerW> layers;
    float* bias_tab = nullptr;  // [heads][2*maxL-1]
    int* bucket_dev = nullptr;
    bool weights_ready = false;
    // activations (capacity in tokens / sequences)
    int cap_tokens = 0, cap_seqs = 0, num_cus = 256;
    float *x32 = nullptr, *pre32 = nullptr;          // [T, H] fp32
    void *x16 = nullptr, *qkv = nullptr, *ctx = nullptr, *ffn = nullptr;  // operand-typed
    long long* stats[2] = {nullptr, nullptr};        // [T][2] fixed-point row sums of the two pre tensors (folded-LN path)
    bool x32_valid = true;                           // false after a folded-LN forward (x32 is not materialised there)
    float att_range = 1.2676506e30f;                 // 2^100: row-sum range of the reference-free softmax pass (attn_pass); 0 = always the SAFE pass
    int32_t *ids_dev = nullptr, *cu_dev = nullptr;
    float* out_dev = nullptr;
    // css_encoder_forward_spans: span table [S][3], span rows [S, H], scores [S], query [H].  Grow-only and apart from
    // the buffers above: no captured graph holds one of these pointers, so growing them leaves the graphs alone.
    int cap_spans = 0;
    int32_t* spans_dev = nullptr;
    float *span_out_dev = nullptr, *span_scores_dev = nullptr, *span_q_dev = nullptr;
    // css_encoder_set_head / css_encoder_forward_pairs: head weights [H*H + H + H + 1] (Wp, bp, wc, bc), segment starts
    // [B], logits [B].  Grow-only and apart from the activations, like the span buffers: no graph holds them.
    float* head_dev = nullptr;
    bool head_set = false;
    int cap_pairs = 0;
    int32_t* seg_dev = nullptr;
    float* logits_dev = nullptr;
    // css_encoder_set_token_projection / css_encoder_forward_tokens / css_encoder_maxsim: projection [P][H] fp32
    // (tok_p == 0: none, the token vectors are the hidden states), and the host entry points' device copies: token
    // rows, query rows, both offset tables, keep flags, pairs, scores.  Grow-only and apart from the activations, like
    // the span buffers: no graph holds them.
    float* tokw_dev = nullptr;
    int tok_p = 0;
    css::DevBuf<bf16_t> li_tok, li_q;
    css::DevBuf<int32_t> li_cuq, li_cud, li_pairs;
    css::DevBuf<uint8_t> li_keep;
    css::DevBuf<float> li_scores, li_part;   // li_part: partial maxima [np][nsplit][64] of a split MaxSim launch
    // css_encoder_set_mlm_head / css_encoder_forward_sparse / css_encoder_vocab_max: the head's transform
    // [H*H + 3H] fp32 (Wd, bd, LayerNorm gamma, beta) with Wd's bf16 copy for the LayerNorm-folded path, the decoder
    // bias c [V], and the decoder E [V][H] in the operand type of the compute mode (mlm_e32 == wemb: tied, fp32 mode;
    // mlm_e32_own holds an untied fp32 decoder).  sp_*: the host entry points' device copies (token rows, their bf16
    // rounding, offsets) and the results (zmax bit patterns [B][V], terms / weights [B][m], nnz [B]).  Grow-only and
    // apart from the activations, like li_*: no graph holds them.
    css::DevBuf<float> mlm_w, mlm_c, mlm_e32_own;
    css::DevBuf<bf16_t> mlm_wd16, mlm_e16;
    const float* mlm_e32 = nullptr;
    bool mlm_set = false;
    css::DevBuf<float> sp_rows, sp_w;
    css::DevBuf<bf16_t> sp_g16;
    css::DevBuf<int32_t> sp_cu, sp_terms, sp_nnz;
    css::DevBuf<unsigned> sp_z;
    // hipGraph cache for the launch-bound tiny-batch path (generate_single_embedding): key =
    // (B, T, max_len, normalize); a key is run eagerly once, captured on its second use, replayed after
    struct GraphEntry {
        int uses = 0;
        hipGraphExec_t exec = nullptr;
    };
    std::map<uint64_t, GraphEntry> graphs;
    bool graphs_ok = true;
    std::mutex mu;
};

namespace {

int alloc_param(css_encoder* e, const std::string& name, int64_t numel, uint32_t sid, float mean, float std,
                float** out) {
    float* p = nullptr;
    hipError_t err = hipMalloc((void**)&p, (size_t)numel * sizeof(float));
    if (err != hipSuccess) return css::hip_fail(err, "hipMalloc(weights)", __FILE__, __LINE__);
    Param prm;
    prm.p = p;
    prm.numel = numel;
    prm.synth_id = sid;
    prm.mean = mean;
    prm.std = std;
    e->params[name] = prm;
    *out = p;
    return CSS_OK;
}

// The LayerNorm-folded bf16 path (forward_folded_bf16) is built for hidden 768 / head_dim 64 and N % 256 GEMMs.
bool folded_shape(const css_encoder_cfg& c) {
    return c.compute == 0 && c.hidden == 768 && c.heads * 64 == c.hidden && c.ffn % 256 == 0;
}

// HF key names.  q/k/v are views into the fused
// [3H, H] weight / [3H] bias, in that order.  MPNet: transformers' MPNetModel names (the fused tensor may be given
// whole or as its three views); BERT: BertModel names (query / key / value are the only names of the fused rows).
int build_params(css_encoder* e) {
    const css_encoder_cfg& c = e->cfg;
    const int64_t H = c.hidden, F = c.ffn;
    const bool bert = c.arch == CSS_ENCODER_ARCH_BERT;
    int rc;
#define AP(name, n, sid, mean, std, ptr) \
    if ((rc = alloc_param(e, name, n, sid, mean, std, ptr)) != CSS_OK) return rc
    AP("embeddings.word_embeddings.weight", (int64_t)c.vocab * H, 0, 0.f, 0.02f, &e->wemb);
    AP("embeddings.position_embeddings.weight", (int64_t)c.max_pos * H, 1, 0.f, 0.02f, &e->pemb);
    AP("embeddings.LayerNorm.weight", H, 2, 1.f, 0.1f, &e->embg);
    AP("embeddings.LayerNorm.bias", H, 3, 0.f, 0.05f, &e->embb);
    if (bert) {
        AP("embeddings.token_type_embeddings.weight", 2 * H, 5, 0.f, 0.02f, &e->tte);
        CSS_HIP_TRY(hipMalloc((void**)&e->pemb_eff, (size_t)c.max_pos * H * 4));
        e->extra.push_back(e->pemb_eff);
        CSS_HIP_TRY(hipMalloc((void**)&e->tdelta, (size_t)H * 4));
        e->extra.push_back(e->tdelta);
    } else {
        AP("encoder.relative_attention_bias.weight", (int64_t)c.rel_buckets * c.heads, 4, 0.f, 0.1f, &e->relw);
        e->pemb_eff = e->pemb;
    }
    e->layers.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; ++i) {
        LayerW& L = e->layers[i];
        const std::string pre = "encoder.layer." + std::to_string(i) + ".";
        const uint32_t base = 16 + 16 * i;
        if (bert) {
            CSS_HIP_TRY(hipMalloc((void**)&L.wqkv, (size_t)3 * H * H * 4));
            e->extra.push_back(L.wqkv);
            CSS_HIP_TRY(hipMalloc((void**)&L.bqkv, (size_t)3 * H * 4));
            e->extra.push_back(L.bqkv);
            AP(pre + "attention.output.dense.weight", H * H, base + 6, 0.f, 0.02f, &L.wo);
            AP(pre + "attention.output.dense.bias", H, base + 7, 0.f, 0.05f, &L.bo);
            AP(pre + "attention.output.LayerNorm.weight", H, base + 8, 1.f, 0.1f, &L.ln1g);
            AP(pre + "attention.output.LayerNorm.bias", H, base + 9, 0.f, 0.05f, &L.ln1b);
        } else {
            AP(pre + "attention.attn.qkv.weight", 3 * H * H, base + 0, 0.f, 0.02f, &L.wqkv);
            AP(pre + "attention.attn.qkv.bias", 3 * H, base + 1, 0.f, 0.05f, &L.bqkv);
            AP(pre + "attention.attn.o.weight", H * H, base + 6, 0.f, 0.02f, &L.wo);
            AP(pre + "attention.attn.o.bias", H, base + 7, 0.f, 0.05f, &L.bo);
            AP(pre + "attention.LayerNorm.weight", H, base + 8, 1.f, 0.1f, &L.ln1g);
            AP(pre + "attention.LayerNorm.bias", H, base + 9, 0.f, 0.05f, &L.ln1b);
        }
        AP(pre + "intermediate.dense.weight", F * H, base + 10, 0.f, 0.02f, &L.w1);
        AP(pre + "intermediate.dense.bias", F, base + 11, 0.f, 0.05f, &L.b1);
        AP(pre + "output.dense.weight", H * F, base + 12, 0.f, 0.02f, &L.w2);
        AP(pre + "output.dense.bias", H, base + 13, 0.f, 0.05f, &L.b2);
        AP(pre + "output.LayerNorm.weight", H, base + 14, 1.f, 0.1f, &L.ln2g);
        AP(pre + "output.LayerNorm.bias", H, base + 15, 0.f, 0.05f, &L.ln2b);
        // q/k/v views (weights: rows [0,H) [H,2H) [2H,3H) of the fused matrix)
        const char* nm[3] = {"q", "k", "v"};
        const char* bnm[3] = {"query", "key", "value"};
        for (int j = 0; j < 3; ++j) {
            const std::string vn = bert ? pre + "attention.self." + bnm[j] : pre + "attention.attn." + nm[j];
            Param w;
            w.p = L.wqkv + (size_t)j * H * H;
            w.numel = H * H;
            w.synth_id = base + 2 * j;  // MPNet: informational (synthetic init fills the fused tensors); BERT: its seed
            w.owned = false;
            w.synth = bert;
            w.required = bert;
            Param b = w;
            b.p = L.bqkv + (size_t)j * H;
            b.numel = H;
            b.synth_id = base + 2 * j + 1;
            b.mean = 0.f;
            b.std = 0.05f;
            e->params[vn + ".weight"] = w;
            e->params[vn + ".bias"] = b;
        }
        CSS_HIP_TRY(hipMalloc((void**)&L.wqkv_h, (size_t)3 * H * H * 2));
        CSS_HIP_TRY(hipMalloc((void**)&L.wo_h, (size_t)H * H * 2));
        CSS_HIP_TRY(hipMalloc((void**)&L.w1_h, (size_t)F * H * 2));
        CSS_HIP_TRY(hipMalloc((void**)&L.w2_h, (size_t)H * F * 2));
        if (folded_shape(c)) {
            CSS_HIP_TRY(hipMalloc((void**)&L.wqkv_f, (size_t)3 * H * H * 2));
            CSS_HIP_TRY(hipMalloc((void**)&L.w1_f, (size_t)F * H * 2));
            CSS_HIP_TRY(hipMalloc((void**)&L.w2_p, (size_t)H * F * 2));
            CSS_HIP_TRY(hipMalloc((void**)&L.wo_p, (size_t)H * H * 2));
            CSS_HIP_TRY(hipMalloc((void**)&L.dqkv, (size_t)3 * H * 4));
            CSS_HIP_TRY(hipMalloc((void**)&L.d1, (size_t)F * 4));
            CSS_HIP_TRY(hipMalloc((void**)&L.bo_f, (size_t)H * 4));
            CSS_HIP_TRY(hipMalloc((void**)&L.b2_f, (size_t)H * 4));
        }
    }
#undef AP
    if (bert) return CSS_OK;   // no relative position bias
    const int maxL = c.max_seq_len;
    CSS_HIP_TRY(hipMalloc((void**)&e->bias_tab, (size_t)c.heads * (2 * maxL - 1) * sizeof(float)));
    CSS_HIP_TRY(hipMalloc((void**)&e->bucket_dev, (size_t)(2 * maxL - 1) * sizeof(int)));
    std::vector<int> bucket(2 * maxL - 1);
    for (int r = 0; r < 2 * maxL - 1; ++r) bucket[r] = css_mpnet_rel_bucket(r - (maxL - 1), c.rel_buckets, 128);
    CSS_HIP_TRY(hipMemcpy(e->bucket_dev, bucket.data(), bucket.size() * sizeof(int), hipMemcpyHostToDevice));
    return CSS_OK;
}

// After the fp32 masters change: bf16 operand copies + the per-head Toeplitz bias table.
int finalize_weights(css_encoder* e) {
    const css_encoder_cfg& c = e->cfg;
    const size_t H = c.hidden, F = c.ffn;
    hipStream_t st = e->stream;
    for (size_t li = 0; li < e->layers.size(); ++li) {
        LayerW& L = e->layers[li];
        if (L.wqkv_f) {
            const float* g_in = li == 0 ? e->embg : e->layers[li - 1].ln2g;
            const float* b_in = li == 0 ? e->embb : e->layers[li - 1].ln2b;
            hipLaunchKernelGGL(k_fold_ln, dim3((3 * H + 3) / 4), dim3(256), 0, st, L.wqkv, g_in, b_in, L.bqkv, (int)(3 * H),
                               (int)H, L.wqkv_f, L.dqkv, 1);
            hipLaunchKernelGGL(k_fold_ln, dim3((F + 3) / 4), dim3(256), 0, st, L.w1, L.ln1g, L.ln1b, L.b1, (int)F, (int)H,
                               L.w1_f, L.d1, 1);
            hipLaunchKernelGGL(k_add_vec, dim3((H + 255) / 256), dim3(256), 0, st, L.bo, b_in, L.bo_f, (int)H);
            hipLaunchKernelGGL(k_add_vec, dim3((H + 255) / 256), dim3(256), 0, st, L.b2, L.ln1b, L.b2_f, (int)H);
            hipLaunchKernelGGL(k_f32_to_bf16_kperm, dim3(1024), dim3(256), 0, st, L.w2, L.w2_p, H * F, (int)F);
            hipLaunchKernelGGL(k_f32_to_bf16_kperm, dim3(1024), dim3(256), 0, st, L.wo, L.wo_p, H * H, (int)H);
        }
    }
    for (auto& L : e->layers) {
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, st, L.wqkv, L.wqkv_h, 3 * H * H);
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, st, L.wo, L.wo_h, H * H);
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, st, L.w1, L.w1_h, F * H);
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, st, L.w2, L.w2_h, H * F);
    }
    if (c.arch == CSS_ENCODER_ARCH_BERT) {
        const size_t n = (size_t)c.max_pos * H;
        hipLaunchKernelGGL(k_add_row, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, e->pemb, e->tte, e->pemb_eff,
                           c.max_pos, (int)H);
        hipLaunchKernelGGL(k_type_delta, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, e->tte, e->tdelta, (int)H);
    } else {
        const int n = c.heads * (2 * c.max_seq_len - 1);
        hipLaunchKernelGGL(k_build_bias_tab, dim3((n + 255) / 256), dim3(256), 0, st, e->relw, e->bucket_dev, c.heads,
                           c.max_seq_len, c.compute == 0 ? 1.44269504088896341f : 1.0f, e->bias_tab);
    }
    CSS_LAUNCH_CHECK();
    CSS_HIP_TRY(hipStreamSynchronize(st));
    e->weights_ready = true;
    return CSS_OK;
}

int ensure_acts(css_encoder* e, int T, int B) {
    const css_encoder_cfg& c = e->cfg;
    const size_t H = c.hidden, F = c.ffn;
    const size_t es = c.compute == 0 ? 2 : 4;
    T = std::max(T, 8 * B);  // pre32 also holds the [B][8][H] pooling partials
    if (T > e->cap_tokens || B > e->cap_seqs) {
        for (auto& kv : e->graphs)
            if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        e->graphs.clear();  // captured pointers are about to change
    }
    if (T > e->cap_tokens) {
        void* ptrs[] = {e->x32, e->pre32, e->x16, e->qkv, e->ctx, e->ffn, e->ids_dev, e->stats[0], e->stats[1]};
        for (void* p : ptrs)
            if (p) CSS_HIP_TRY(hipFree(p));
        e->cap_tokens = 0;
        // GEMM tiles store whole 256-row tiles unconditionally: keep >= 256 slack rows
        const size_t cap = ((size_t)T + 255) / 256 * 256 + 256;
        CSS_HIP_TRY(hipMalloc((void**)&e->x32, cap * H * 4));
        CSS_HIP_TRY(hipMalloc((void**)&e->pre32, cap * H * 4));
        // (+ cap * 64 bytes: the padding of the blocked layout the LayerNorm-folded path keeps in x16 / pre32 / ffn)
        CSS_HIP_TRY(hipMalloc((void**)&e->x16, cap * H * es + cap * 64));
        CSS_HIP_TRY(hipMalloc((void**)&e->qkv, cap * 3 * H * es));
        CSS_HIP_TRY(hipMalloc((void**)&e->ctx, cap * H * es));
        CSS_HIP_TRY(hipMalloc((void**)&e->ffn, cap * F * es + cap * 64));
        CSS_HIP_TRY(hipMalloc((void**)&e->ids_dev, cap * sizeof(int32_t)));
        e->stats[0] = e->stats[1] = nullptr;
        if (c.compute == 0) {
            for (int i = 0; i < 2; ++i) {
                CSS_HIP_TRY(hipMalloc((void**)&e->stats[i], cap * 16));
                CSS_HIP_TRY(hipMemset(e->stats[i], 0, cap * 16));  // slack rows: finite values
            }
            // the memsets run on the null stream, forwards on non-blocking streams: order them here, once per growth
            CSS_HIP_TRY(hipDeviceSynchronize());
        }
        e->cap_tokens = (int)cap;
    }
    if (B > e->cap_seqs) {
        if (e->cu_dev) CSS_HIP_TRY(hipFree(e->cu_dev));
        if (e->out_dev) CSS_HIP_TRY(hipFree(e->out_dev));
        e->cap_seqs = 0;
        const size_t cap = (size_t)B + 64;
        CSS_HIP_TRY(hipMalloc((void**)&e->cu_dev, (cap + 1) * sizeof(int32_t)));
        CSS_HIP_TRY(hipMalloc((void**)&e->out_dev, cap * H * 4));
        e->cap_seqs = (int)cap;
    }
    return CSS_OK;
}

// Buffers of css_encoder_forward_spans (host entry point).  The stream is idle between calls (every host entry point
// ends with a synchronise), so the old buffers can be freed at once.
int ensure_spans(css_encoder* e, int S) {
    const size_t H = e->cfg.hidden;
    if (!e->span_q_dev) CSS_HIP_TRY(hipMalloc((void**)&e->span_q_dev, H * 4));
    if (S <= e->cap_spans) return CSS_OK;
    void* ptrs[] = {e->spans_dev, e->span_out_dev, e->span_scores_dev};
    for (void* p : ptrs)
        if (p) CSS_HIP_TRY(hipFree(p));
    e->spans_dev = nullptr;
    e->span_out_dev = e->span_scores_dev = nullptr;
    e->cap_spans = 0;
    const size_t cap = (size_t)S + (size_t)S / 2 + 64;
    CSS_HIP_TRY(hipMalloc((void**)&e->spans_dev, cap * 3 * sizeof(int32_t)));
    CSS_HIP_TRY(hipMalloc((void**)&e->span_out_dev, cap * H * 4));
    CSS_HIP_TRY(hipMalloc((void**)&e->span_scores_dev, cap * 4));
    e->cap_spans = (int)cap;
    return CSS_OK;
}

// Tile shapes: 2x2 waves x (2x2) MFMA tiles = 128x128, or 2x4 waves x (4x2) tiles = 256x256
// (8 waves, 128 KiB ring).  Persistent: one block per CU (grid a multiple of 8).
template <typename TIn, int EPI, int WM, int WN, int TM, int TN, int NST, int RB, int SPS>
int launch_gemm_t(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int qscale_cols,
                  float qscale, int num_cus, hipStream_t st, const char* prof) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    CSS_REQUIRE(N % BN == 0 && K % 64 == 0 && K / 64 >= 3, "gemm: N=%d must be a multiple of %d and K=%d of 64 (>= 192)", N, BN, K);
    const int ntn = N / BN, ntm = (M + BM - 1) / BM;
    auto kern = k_gemm<TIn, EPI, WM, WN, TM, TN, NST, RB, SPS>;
    const size_t lds = (size_t)NST * (BM + BN) * RB;  // ring of NST stages, RB bytes of K per row
    int dev_ = 0;
    (void)hipGetDevice(&dev_);
    int rc_ = css::ensure_dynamic_lds((const void*)kern, lds, dev_);   // (mutex-protected, once per kernel and device)
    if (rc_ != CSS_OK) return rc_;
    const int blocks_per_cu = lds <= 80 * 1024 ? 2 : 1;
    int grid = std::min(ntn * ntm, num_cus * blocks_per_cu);
    grid = std::max(8, grid / 8 * 8);
    ProfScope ps(prof, st);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WM * WN * 64), lds, st, (const TIn*)A, (const TIn*)W, bias, C, M, N, K,
                       qscale_cols, qscale);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// k_gemm8p launch (256x256 tiles, persistent, one block per CU); `side` carries the LayerNorm-folding operands
template <int EPI, bool ABLK = false, int TAG = 0>
int launch_gemm8p(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int qscale_cols,
                  float qscale, const G8Side& side, int num_cus, hipStream_t st, const char* prof) {
    CSS_REQUIRE(N % 256 == 0 && K % 128 == 0 && (size_t)M * K * 2 < ((size_t)1 << 32), "gemm8p: bad shape %d x %d x %d", M, N, K);
    CSS_REQUIRE(EPI != EPI_RES || K >= 256, "gemm8p: EPI_RES needs K >= 256 (statistics are flushed in a tile's third K step)");
    auto kern = k_gemm8p<EPI, ABLK, TAG>;
    constexpr size_t lds = 2 * 4 * G8_HT;
    int dev_ = 0;
    (void)hipGetDevice(&dev_);
    int rc_ = css::ensure_dynamic_lds((const void*)kern, lds, dev_);
    if (rc_ != CSS_OK) return rc_;
    const int ntiles = (N / 256) * ((M + 255) / 256);
    int grid = std::min(ntiles, num_cus);
    grid = std::max(8, grid / 8 * 8);
    ProfScope ps(prof, st);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, (const bf16_t*)A, (const bf16_t*)W, bias, (bf16_t*)C, M, N, K,
                       qscale_cols, qscale, side);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <typename TIn, int EPI>
int launch_gemm(const void* A, const void* W, const float* bias, void* C, int M, int N, int K, int qscale_cols,
                float qscale, int num_cus, hipStream_t st, const char* prof) {
    if (M <= 64 && N % 32 == 0 && K % 384 == 0) {  // single-query / tiny batches: weight-streaming kernel (K/4 = 12n fragment steps)
        ProfScope ps(prof, st);
        // K % 768 == 0: groups of 12 fragment steps; K = 384 (hidden 384: 6 bf16 / 12 fp32 steps per wave): groups of 6
        if (K % 768 == 0) {
            if (M <= 32)
                hipLaunchKernelGGL((k_gemm_skinny<TIn, EPI, 1>), dim3(N / 32), dim3(256), 0, st, (const TIn*)A, (const TIn*)W,
                                   bias, C, M, N, K, qscale_cols, qscale);
            else
                hipLaunchKernelGGL((k_gemm_skinny<TIn, EPI, 2>), dim3(N / 32), dim3(256), 0, st, (const TIn*)A, (const TIn*)W,
                                   bias, C, M, N, K, qscale_cols, qscale);
        } else {
            if (M <= 32)
                hipLaunchKernelGGL((k_gemm_skinny<TIn, EPI, 1, 6>), dim3(N / 32), dim3(256), 0, st, (const TIn*)A,
                                   (const TIn*)W, bias, C, M, N, K, qscale_cols, qscale);
            else
                hipLaunchKernelGGL((k_gemm_skinny<TIn, EPI, 2, 6>), dim3(N / 32), dim3(256), 0, st, (const TIn*)A,
                                   (const TIn*)W, bias, C, M, N, K, qscale_cols, qscale);
        }
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    if (M >= 1024 && N % 256 == 0) {
        // ring: 2 stages x 128 B rows.  Rings of 3 / 4 x 64 B rows and 5 x 64 B with two stages per step were
        // measured slower (more barriers, same LDS fill rate) and are not kept.
        if constexpr (sizeof(TIn) == 2) {
            static_assert(EPI == EPI_QKV || EPI == EPI_GELU, "bf16 GEMMs write bf16 rows");
            if (K % 128 == 0 && (size_t)M * K * 2 < ((size_t)1 << 32))
                return launch_gemm8p<EPI>(A, W, bias, C, M, N, K, qscale_cols, qscale, G8Side{}, num_cus, st, prof);
            // the 16x16x32 MFMA variant: the chip holds a higher clock under it than under 32x32x16
            CSS_REQUIRE(K % 64 == 0 && K / 64 >= 3, "gemm: K=%d must be a multiple of 64 (>= 192)", K);
            auto kern = k_gemm16<EPI>;
            constexpr size_t lds = 2 * 512 * 128;
            int dev_ = 0;
            (void)hipGetDevice(&dev_);
            int rc_ = css::ensure_dynamic_lds((const void*)kern, lds, dev_);
            if (rc_ != CSS_OK) return rc_;
            const int ntiles = (N / 256) * ((M + 255) / 256);
            int grid = std::min(ntiles, num_cus);
            grid = std::max(8, grid / 8 * 8);
            ProfScope ps(prof, st);
            hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, (const bf16_t*)A, (const bf16_t*)W, bias, C, M, N, K,
                               qscale_cols, qscale);
            CSS_LAUNCH_CHECK();
            return CSS_OK;
        } else {
            return launch_gemm_t<TIn, EPI, 2, 4, 4, 2, 2, 128, 1>(A, W, bias, C, M, N, K, qscale_cols, qscale, num_cus, st, prof);
        }
    }
    return launch_gemm_t<TIn, EPI, 2, 2, 2, 2, 4, 64, 1>(A, W, bias, C, M, N, K, qscale_cols, qscale, num_cus, st, prof);
}

// Position id of a sequence's first token: MPNet padding_idx + 1 (cumsum(mask) * mask + padding_idx), BERT 0.
int pos_offset(const css_encoder_cfg& c) { return c.arch == CSS_ENCODER_ARCH_BERT ? 0 : 2; }

// Softmax scale 1 / sqrt(head_dim), folded into the q columns of the QKV GEMM (bf16: times log2(e), exp2 softmax).
float qk_scale(const css_encoder_cfg& c, bool bf) {
    const float s = 1.0f / std::sqrt((float)(c.hidden / c.heads));   // exactly 0.125 at head_dim 64
    return bf ? s * 1.44269504088896341f : s;
}

template <int HD, bool BLK, bool BIAS>
void launch_attention_bf16_t(css_encoder* e, const int32_t* cu, int B, int max_len, hipStream_t st) {
    const int maxL = e->cfg.max_seq_len;
    const size_t lds = 4 * 8192 + (BIAS ? (size_t)(2 * maxL - 1 + 64) * 4 : 0);
    const int nqb = (max_len + 127) / 128;
    hipLaunchKernelGGL((k_attention_bf16<HD, BLK, BIAS>), dim3(B * nqb * e->cfg.heads), dim3(256), lds, st,
                       (const bf16_t*)e->qkv, cu, e->bias_tab, maxL, e->cfg.hidden, (bf16_t*)e->ctx, nqb, e->cfg.heads,
                       e->att_range);
}

// bf16 attention of the architecture: MPNet (head_dim 64, relative bias), BERT (head_dim 64 or 32, no bias)
template <bool BLK>
void launch_attention_bf16(css_encoder* e, const int32_t* cu, int B, int max_len, hipStream_t st) {
    if (e->cfg.arch != CSS_ENCODER_ARCH_BERT) launch_attention_bf16_t<64, BLK, true>(e, cu, B, max_len, st);
    else if (e->cfg.hidden / e->cfg.heads == 64) launch_attention_bf16_t<64, BLK, false>(e, cu, B, max_len, st);
    else if constexpr (!BLK) launch_attention_bf16_t<32, false, false>(e, cu, B, max_len, st);
}

template <typename TIn, int H>
int forward_typed(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int T, int max_len, int normalize,
                  float* out, hipStream_t st, const int32_t* seg, int pooling) {
    const css_encoder_cfg& c = e->cfg;
    const int F = c.ffn;
    constexpr bool BF = sizeof(TIn) == 2;
    int rc;
    {
        ProfScope ps("enc_embed_ln", st);
        hipLaunchKernelGGL(k_embed_ln<H>, dim3((T + 3) / 4), dim3(256), 0, st, ids, cu, B, e->wemb, e->pemb_eff,
                           e->embg, e->embb, c.ln_eps, c.vocab, c.max_pos, pos_offset(c), e->x32,
                           BF ? (bf16_t*)e->x16 : nullptr, T, seg, e->tdelta);
        CSS_LAUNCH_CHECK();
    }
    const int maxL = c.max_seq_len;
    // Residual stream storage: fp32 rows (x32) and fp32 branch outputs in fp32 mode; in bf16 mode both are bf16
    // (the residual is the row the next GEMM reads anyway).
    // attention-output / FFN2 projection into `pre32` (fp32, or bf16 rows in bf16 mode)
    auto launch_branch_out = [&](const void* a, const void* w, const float* bias, int K, const char* prof) -> int {
        if constexpr (BF) return launch_gemm<TIn, EPI_QKV>(a, w, bias, e->pre32, T, H, K, 0, 1.0f, e->num_cus, st, prof);
        else return launch_gemm<TIn, EPI_RESID>(a, w, bias, e->pre32, T, H, K, 0, 1.0f, e->num_cus, st, prof);
    };
    // x = LN(pre + x); `last`: the fp32 row is needed by the pooling
    auto launch_ln = [&](const float* g, const float* b, bool last) -> int {
        ProfScope ps("enc_layernorm", st);
        const dim3 grid((T + 3) / 4), blk(256);
        if constexpr (BF)
            hipLaunchKernelGGL((k_layernorm<H, bf16_t, bf16_t>), grid, blk, 0, st, (const bf16_t*)e->pre32, (const bf16_t*)e->x16, g, b,
                               c.ln_eps, last ? e->x32 : (float*)nullptr, (bf16_t*)e->x16, T);
        else
            hipLaunchKernelGGL((k_layernorm<H, float, float>), grid, blk, 0, st, (const float*)e->pre32, (const float*)e->x32, g, b,
                               c.ln_eps, e->x32, (bf16_t*)nullptr, T);
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    };
    for (int li = 0; li < c.num_layers; ++li) {
        const LayerW& L = e->layers[li];
        const void* xin = BF ? e->x16 : (const void*)e->x32;
        const void* wqkv = BF ? (const void*)L.wqkv_h : (const void*)L.wqkv;
        if ((rc = launch_gemm<TIn, EPI_QKV>(xin, wqkv, L.bqkv, e->qkv, T, 3 * H, H, H, qk_scale(c, BF), e->num_cus, st, "enc_gemm_qkv")) != CSS_OK)
            return rc;
        {
            ProfScope ps("enc_attention", st);
            if constexpr (BF) {
                launch_attention_bf16<false>(e, cu, B, max_len, st);
            } else if (H / c.heads == 64) {
                hipLaunchKernelGGL(k_attention_f32<64>, dim3(B, max_len, c.heads), dim3(64), 0, st, (const float*)e->qkv, cu,
                                   e->bias_tab, maxL, H, (float*)e->ctx);
            } else {
                hipLaunchKernelGGL(k_attention_f32<32>, dim3(B, max_len, c.heads), dim3(64), 0, st, (const float*)e->qkv, cu,
                                   e->bias_tab, maxL, H, (float*)e->ctx);
            }
            CSS_LAUNCH_CHECK();
        }
        const void* wo = BF ? (const void*)L.wo_h : (const void*)L.wo;
        if ((rc = launch_branch_out(e->ctx, wo, L.bo, H, "enc_gemm_o")) != CSS_OK) return rc;
        if ((rc = launch_ln(L.ln1g, L.ln1b, false)) != CSS_OK) return rc;
        xin = BF ? e->x16 : (const void*)e->x32;
        const void* w1 = BF ? (const void*)L.w1_h : (const void*)L.w1;
        if ((rc = launch_gemm<TIn, EPI_GELU>(xin, w1, L.b1, e->ffn, T, F, H, 0, 1.0f, e->num_cus, st, "enc_gemm_ffn1")) != CSS_OK)
            return rc;
        const void* w2 = BF ? (const void*)L.w2_h : (const void*)L.w2;
        if ((rc = launch_branch_out(e->ffn, w2, L.b2, F, "enc_gemm_ffn2")) != CSS_OK) return rc;
        if ((rc = launch_ln(L.ln2g, L.ln2b, li == c.num_layers - 1)) != CSS_OK) return rc;
    }
    {
        ProfScope ps("enc_pool", st);
        constexpr int kPoolSlices = 8;
        if (pooling == CSS_ENCODER_POOL_CLS) {
            hipLaunchKernelGGL(k_pool_cls<H>, dim3(B), dim3(256), 0, st, e->x32, cu, normalize, out);
        } else {
            // partial sums live in pre32 (free after the last LayerNorm): [B][8][H] floats
            hipLaunchKernelGGL(k_pool_partial<H>, dim3(B, kPoolSlices), dim3(256), 0, st, e->x32, cu, kPoolSlices, e->pre32);
            hipLaunchKernelGGL(k_pool_final<H>, dim3(B), dim3(256), 0, st, e->pre32, cu, kPoolSlices, normalize, out);
        }
        CSS_LAUNCH_CHECK();
    }
    return CSS_OK;
}

// bf16 product path for batches of >= 1024 tokens: LayerNorm folded into the GEMM epilogues (css_encoder_kernels.h,
// "LayerNorm without LayerNorm kernels").  Launches per layer: QKV GEMM, attention, O GEMM, FFN1 GEMM, FFN2 GEMM.
// The two pre tensors alternate between x16 and pre32 (both hold bf16 rows here).
int forward_folded_bf16(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int T, int max_len, int normalize,
                        float* out, hipStream_t st, const int32_t* seg, int pooling) {
    const css_encoder_cfg& c = e->cfg;
    const int H = c.hidden, F = c.ffn;
    int rc;
    bf16_t* pre[2] = {(bf16_t*)e->x16, (bf16_t*)e->pre32};
    {
        ProfScope ps("enc_embed_ln", st);
        hipLaunchKernelGGL(k_embed_pre<768>, dim3((T + 15) / 16), dim3(256), 0, st, ids, cu, B, e->wemb, e->pemb_eff, c.vocab,
                           c.max_pos, pos_offset(c), pre[0], e->stats[0], T, kStatScale1, kStatScale2, seg, e->tdelta);
        CSS_LAUNCH_CHECK();
    }
    const float *g_in = e->embg, *b_in = e->embb;  // the LayerNorm that turns pre[0] into the layer input
    G8Side side{};
    side.inv_h = 1.0f / H;
    side.eps = c.ln_eps;
    for (int li = 0; li < c.num_layers; ++li) {
        const LayerW& L = e->layers[li];
        // x = LN(pre[0]) -> qkv; zeroes stats[1]
        side.stats_in = e->stats[0];
        side.stats_out = e->stats[1];
        if ((rc = launch_gemm8p<EPI_AFF_QKV, true>(pre[0], L.wqkv_f, L.dqkv, e->qkv, T, 3 * H, H, H, qk_scale(c, true),
                                                   side, e->num_cus, st, "enc_gemm_qkv")) != CSS_OK)
            return rc;
        {
            ProfScope ps("enc_attention", st);
            launch_attention_bf16<true>(e, cu, B, max_len, st);
            CSS_LAUNCH_CHECK();
        }
        // pre[1] = ctx Wo^T + (bo + beta) + gamma (pre[0] - mu) rs; stats[1] += row sums
        side.pprev = pre[0];
        side.cvec = g_in;
        if ((rc = launch_gemm8p<EPI_RES, true, 1>(e->ctx, L.wo_p, L.bo_f, pre[1], T, H, H, 0, 1.0f, side, e->num_cus, st, "enc_gemm_o")) != CSS_OK)
            return rc;
        // x1 = LN1(pre[1]) -> ffn = gelu(x1 W1^T + b1); zeroes stats[0]
        side.stats_in = e->stats[1];
        side.stats_out = e->stats[0];
        if ((rc = launch_gemm8p<EPI_AFF_GELU, true>(pre[1], L.w1_f, L.d1, e->ffn, T, F, H, 0, 1.0f, side, e->num_cus, st, "enc_gemm_ffn1")) != CSS_OK)
            return rc;
        // pre[0] = ffn W2^T + (b2 + beta1) + gamma1 (pre[1] - mu) rs; stats[0] += row sums
        side.pprev = pre[1];
        side.cvec = L.ln1g;
        if ((rc = launch_gemm8p<EPI_RES, true>(e->ffn, L.w2_p, L.b2_f, pre[0], T, H, F, 0, 1.0f, side, e->num_cus, st, "enc_gemm_ffn2")) != CSS_OK)
            return rc;
        g_in = L.ln2g;
        b_in = L.ln2b;
    }
    {
        ProfScope ps("enc_pool", st);
        constexpr int kPoolSlices = 8;
        // partial sums live in ffn (free after the last FFN2; capacity >= 8 B rows of 8 H bytes): [B][8][H] floats
        float* part = (float*)e->ffn;
        if (pooling == CSS_ENCODER_POOL_CLS) {
            hipLaunchKernelGGL(k_pool_cls_ln<768>, dim3(B), dim3(256), 0, st, (const bf16_t*)pre[0], e->stats[0], g_in, b_in,
                               1.0f / H, c.ln_eps, cu, normalize, out);
        } else {
            hipLaunchKernelGGL(k_pool_partial_ln<768>, dim3(B, kPoolSlices), dim3(256), 0, st, (const bf16_t*)pre[0], e->stats[0],
                               g_in, b_in, 1.0f / H, c.ln_eps, cu, kPoolSlices, part);
            hipLaunchKernelGGL(k_pool_final<768>, dim3(B), dim3(256), 0, st, part, cu, kPoolSlices, normalize, out);
        }
        CSS_LAUNCH_CHECK();
    }
    e->x32_valid = false;
    return CSS_OK;
}

// seg (pair batches: per-sequence segment start, else NULL) and pooling (cfg.pooling, or CLS for the pair head) are the
// only things a pair forward changes; with seg == NULL every kernel does what it does for css_encoder_forward.
int forward_any(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int T, int max_len, int normalize,
                float* out, hipStream_t st, const int32_t* seg = nullptr, int pooling = -1) {
    if (pooling < 0) pooling = e->cfg.pooling;
    if (!e->weights_ready) {
        css::set_error("css_encoder_forward: weights not loaded (call css_encoder_load_weights or css_encoder_init_synthetic)");
        return CSS_ERR_STATE;
    }
    CSS_REQUIRE(B >= 1 && T >= B, "css_encoder_forward: bad batch (B=%d, tokens=%d)", B, T);
    CSS_REQUIRE(max_len >= 1 && max_len <= e->cfg.max_seq_len, "css_encoder_forward: max_len=%d outside [1, %d]", max_len,
                e->cfg.max_seq_len);
    // Hidden 384 (BERT small: GEMM N in {384, 1152, 1536}, K in {384, 1536}) always takes the unfolded path: its GEMMs
    // run on the 128x128 k_gemm tile (k_gemm8p for N = 1536) and k_gemm_skinny for <= 64 tokens.
    if (folded_shape(e->cfg) && T >= 1024 && (size_t)T * e->cfg.ffn * 2 < ((size_t)1 << 32))
        return forward_folded_bf16(e, ids, cu, B, T, max_len, normalize, out, st, seg, pooling);
    e->x32_valid = true;
    if (e->cfg.hidden == 384)
        return e->cfg.compute == 0 ? forward_typed<bf16_t, 384>(e, ids, cu, B, T, max_len, normalize, out, st, seg, pooling)
                                   : forward_typed<float, 384>(e, ids, cu, B, T, max_len, normalize, out, st, seg, pooling);
    return e->cfg.compute == 0 ? forward_typed<bf16_t, 768>(e, ids, cu, B, T, max_len, normalize, out, st, seg, pooling)
                               : forward_typed<float, 768>(e, ids, cu, B, T, max_len, normalize, out, st, seg, pooling);
}

// One pooled row per span over the token rows that the forward just enqueued on `st` left behind: x32 on the unfolded
// paths, the last pre tensor + its row statistics on the LayerNorm-folded one (pre[0] = x16, stats[0]: the pooling
// kernels only read them).  One launch.
int pool_spans(css_encoder* e, const int32_t* cu, int B, const int32_t* spans, int S, const float* q, int normalize,
               float* span_out, float* scores, hipStream_t st) {
    if (S == 0 || (!span_out && !scores)) return CSS_OK;
    const css_encoder_cfg& c = e->cfg;
    if (!scores) q = nullptr;
    ProfScope ps("enc_span_pool", st);
    if (!e->x32_valid) {
        const LayerW& L = e->layers.back();
        hipLaunchKernelGGL(k_span_pool_ln<768>, dim3(S), dim3(256), 0, st, (const bf16_t*)e->x16, e->stats[0], L.ln2g, L.ln2b,
                           1.0f / c.hidden, c.ln_eps, cu, B, spans, normalize, q, span_out, scores);
    } else if (c.hidden == 384) {
        hipLaunchKernelGGL(k_span_pool<384>, dim3(S), dim3(256), 0, st, e->x32, cu, B, spans, normalize, q, span_out, scores);
    } else {
        hipLaunchKernelGGL(k_span_pool<768>, dim3(S), dim3(256), 0, st, e->x32, cu, B, spans, normalize, q, span_out, scores);
    }
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Buffers of css_encoder_forward_pairs (host entry point); the stream is idle between calls, as for ensure_spans.
int ensure_pairs(css_encoder* e, int B) {
    if (B <= e->cap_pairs) return CSS_OK;
    if (e->seg_dev) CSS_HIP_TRY(hipFree(e->seg_dev));
    if (e->logits_dev) CSS_HIP_TRY(hipFree(e->logits_dev));
    e->seg_dev = nullptr;
    e->logits_dev = nullptr;
    e->cap_pairs = 0;
    const size_t cap = (size_t)B + (size_t)B / 2 + 64;
    CSS_HIP_TRY(hipMalloc((void**)&e->seg_dev, cap * sizeof(int32_t)));
    CSS_HIP_TRY(hipMalloc((void**)&e->logits_dev, cap * 4));
    e->cap_pairs = (int)cap;
    return CSS_OK;
}

// What a pair forward needs of the encoder: BERT, weights and a head.
int check_pairs_state(const css_encoder* e, const char* fn) {
    CSS_REQUIRE(e->cfg.arch == CSS_ENCODER_ARCH_BERT, "%s: the encoder is not a BERT model (token types and the "
                "classification head exist for arch = BERT only)", fn);
    if (!e->head_set) {
        css::set_error("%s: no classification head (call css_encoder_set_head first)", fn);
        return CSS_ERR_STATE;
    }
    return CSS_OK;
}

// The pair forward on `st`: segment-aware forward, CLS rows without normalisation into out_dev [B][H], then the head
// (k_ce_head: partial logits per slab of pooler rows; k_ce_head_sum: their sum + bc).
int forward_pairs_any(css_encoder* e, const int32_t* ids, const int32_t* cu, const int32_t* seg, int B, int T, int max_len,
                      float* logits, hipStream_t st) {
    int rc = forward_any(e, ids, cu, B, T, max_len, 0, e->out_dev, st, seg, CSS_ENCODER_POOL_CLS);
    if (rc != CSS_OK) return rc;
    const size_t H = e->cfg.hidden;
    const float *wp = e->head_dev, *bp = wp + H * H, *wc = bp + H, *bc = wc + H;
    // partials [tiles][H / kCeSlab][kCeTile] live in pre32 (free after the last LayerNorm / the last FFN2 GEMM;
    // capacity >= 8 B rows of H floats, ensure_acts)
    float* part = e->pre32;
    ProfScope ps("enc_ce_head", st);
    const int nslab = (int)H / kCeSlab;
    const dim3 grid((B + kCeTile - 1) / kCeTile, nslab), blk(256);
    if (H == 384) hipLaunchKernelGGL(k_ce_head<384>, grid, blk, 0, st, e->out_dev, wp, bp, wc, B, part);
    else hipLaunchKernelGGL(k_ce_head<768>, grid, blk, 0, st, e->out_dev, wp, bp, wc, B, part);
    hipLaunchKernelGGL(k_ce_head_sum, dim3((B + 255) / 256), dim3(256), 0, st, part, bc, B, nslab, logits);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Shape checks of a packed host batch (css_encoder_forward, css_encoder_forward_spans); *max_len = the longest sequence.
int check_batch(const css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int* max_len) {
    CSS_REQUIRE(B >= 1, "css_encoder_forward: B < 1");
    CSS_REQUIRE(cu[0] == 0, "css_encoder_forward: cu_seqlens[0] must be 0");
    int ml = 0;
    for (int b = 0; b < B; ++b) {
        const int len = cu[b + 1] - cu[b];
        CSS_REQUIRE(len >= 1 && len <= e->cfg.max_seq_len, "css_encoder_forward: sequence %d has length %d outside [1, %d]", b,
                    len, e->cfg.max_seq_len);
        ml = len > ml ? len : ml;
    }
    const int T = cu[B];
    for (int t = 0; t < T; ++t)
        CSS_REQUIRE(ids[t] >= 0 && ids[t] < e->cfg.vocab && ids[t] != e->cfg.pad_id,
                    "css_encoder_forward: token %d has id %d (outside the vocabulary or the pad id)", t, ids[t]);
    *max_len = ml;
    return CSS_OK;
}

// Width of a token vector: the projection's P, or the hidden size without one.
int token_dim(const css_encoder* e) { return e->tok_p ? e->tok_p : e->cfg.hidden; }

// One bf16 row per token over the rows that the forward just enqueued on `st` left behind (the two layouts of
// pool_spans).  One launch.
int write_tokens(css_encoder* e, int T, int normalize, bf16_t* tok_out, hipStream_t st) {
    const css_encoder_cfg& c = e->cfg;
    const int P = token_dim(e);
    const float* W = e->tok_p ? e->tokw_dev : nullptr;
    ProfScope ps("enc_tok_vec", st);
    const dim3 grid((T + 15) / 16), blk(256);
    if (!e->x32_valid) {
        const LayerW& L = e->layers.back();
        hipLaunchKernelGGL(k_tok_vec_ln<768>, grid, blk, 0, st, (const bf16_t*)e->x16, e->stats[0], L.ln2g, L.ln2b,
                           1.0f / c.hidden, c.ln_eps, T, W, P, normalize, tok_out);
    } else if (c.hidden == 384) {
        hipLaunchKernelGGL(k_tok_vec<384>, grid, blk, 0, st, e->x32, T, W, P, normalize, tok_out);
    } else {
        hipLaunchKernelGGL(k_tok_vec<768>, grid, blk, 0, st, e->x32, T, W, P, normalize, tok_out);
    }
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

bool maxsim_width_ok(int P) { return (P % 32 == 0 && P >= 32 && P <= 128) || P == 384 || P == 768; }

template <int P>
int launch_maxsim_p(const css_encoder* e, const bf16_t* q, const int32_t* cuq, int nq, const bf16_t* d, const int32_t* cud,
                    int nd, const uint8_t* keep, const int32_t* pairs, int np, int nsplit, float* scores, float* part,
                    hipStream_t st) {
    constexpr size_t lds = maxsim_lds_bytes<P>();
    const int rc = css::ensure_dynamic_lds((const void*)k_maxsim<P>, lds, e->device);
    if (rc != CSS_OK) return rc;
    hipLaunchKernelGGL(k_maxsim<P>, dim3(np, nsplit), dim3(256), lds, st, q, cuq, nq, d, cud, nd, keep, pairs, scores, part);
    if (nsplit > 1) hipLaunchKernelGGL(k_maxsim_sum, dim3(np), dim3(64), 0, st, part, nsplit, cuq, nq, pairs, scores);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Blocks per doc: one while the pairs alone give every CU CSS_MAXSIM_BLOCKS_PER_CU blocks, else as many as that takes,
// 8 at the most (a 64-pair re-rank batch would otherwise run on 64 of the CUs).  The partial maxima of a split launch
// live in a buffer of the encoder's that only grows; growing frees the old one, so work that an earlier call enqueued
// on another stream must have finished, as for the activations.  DESIGN.md 3.3d has the measurements.
#ifndef CSS_MAXSIM_BLOCKS_PER_CU
#define CSS_MAXSIM_BLOCKS_PER_CU 2
#endif
constexpr int kMaxsimSplitMax = 8;
int launch_maxsim(css_encoder* e, const bf16_t* q, const int32_t* cuq, int nq, const bf16_t* d, const int32_t* cud,
                  int nd, const uint8_t* keep, const int32_t* pairs, int np, int P, float* scores, hipStream_t st) {
    if (np == 0) return CSS_OK;
    const int want = CSS_MAXSIM_BLOCKS_PER_CU * e->num_cus;
    const int nsplit = std::min(kMaxsimSplitMax, std::max(1, (want + np - 1) / np));
    if (nsplit > 1) {
        const int rc = e->li_part.grow((size_t)np * nsplit * kMaxsimQ);
        if (rc != CSS_OK) return rc;
    }
    ProfScope ps("enc_maxsim", st);
    switch (P) {
#define MS(W_) case W_: return launch_maxsim_p<W_>(e, q, cuq, nq, d, cud, nd, keep, pairs, np, nsplit, scores, e->li_part.p, st)
        MS(32); MS(64); MS(96); MS(128); MS(384); MS(768);
#undef MS
    }
    css::set_error("css_encoder_maxsim: P=%d must be a multiple of 32 in [32, 128], or 384, or 768", P);
    return CSS_ERR_INVALID;
}

// Host tables of a MaxSim call, checked before anything is enqueued: every query has 1..64 tokens, every doc at least
// one token and one kept token, every pair names a query and a doc.
int check_maxsim(const char* fn, const int32_t* cuq, int nq, const int32_t* cud, int nd, const uint8_t* keep,
                 const int32_t* pairs, int np) {
    CSS_REQUIRE(nq >= 1 && nd >= 1 && np >= 0, "%s: need nq >= 1, nd >= 1, np >= 0 (got %d, %d, %d)", fn, nq, nd, np);
    CSS_REQUIRE(np == 0 || pairs, "%s: pairs is NULL", fn);
    CSS_REQUIRE(cuq[0] == 0 && cud[0] == 0, "%s: cu_q[0] and cu_d[0] must be 0", fn);
    for (int i = 0; i < nq; ++i) {
        const int m = cuq[i + 1] - cuq[i];
        CSS_REQUIRE(m >= 1 && m <= kMaxsimQ, "%s: query %d has %d tokens, outside [1, %d]", fn, i, m, kMaxsimQ);
    }
    for (int j = 0; j < nd; ++j) {
        const int m = cud[j + 1] - cud[j];
        CSS_REQUIRE(m >= 1, "%s: doc %d has %d tokens (need at least 1)", fn, j, m);
        if (!keep) continue;
        bool any = false;
        for (int t = cud[j]; t < cud[j + 1] && !any; ++t) any = keep[t] != 0;
        CSS_REQUIRE(any, "%s: doc %d has no kept token (d_keep is 0 for all of its %d tokens)", fn, j, m);
    }
    for (int p = 0; p < np; ++p)
        CSS_REQUIRE(pairs[2 * p] >= 0 && pairs[2 * p] < nq && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < nd,
                    "%s: pair %d is (query %d, doc %d), outside [0, %d) x [0, %d)", fn, p, pairs[2 * p], pairs[2 * p + 1], nq, nd);
    return CSS_OK;
}

// Device copies of the query side of a host MaxSim call (query rows, their offsets, keep flags over `nkeep` doc tokens,
// pairs) and room for the scores.  The stream is idle between calls, as for ensure_spans.
int upload_maxsim(css_encoder* e, const uint16_t* q_tok, const int32_t* cuq, int nq, const uint8_t* keep, size_t nkeep,
                  const int32_t* pairs, int np, int P, hipStream_t st) {
    const size_t nqt = (size_t)cuq[nq] * P;
    int rc;
    if ((rc = e->li_q.grow(nqt)) != CSS_OK || (rc = e->li_cuq.grow((size_t)nq + 1)) != CSS_OK ||
        (rc = e->li_pairs.grow((size_t)2 * std::max(np, 1))) != CSS_OK || (rc = e->li_scores.grow(std::max(np, 1))) != CSS_OK ||
        (keep && (rc = e->li_keep.grow(nkeep)) != CSS_OK))
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(e->li_q.p, q_tok, nqt * 2, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->li_cuq.p, cuq, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, st));
    if (np) CSS_HIP_TRY(hipMemcpyAsync(e->li_pairs.p, pairs, (size_t)np * 8, hipMemcpyHostToDevice, st));
    if (keep) CSS_HIP_TRY(hipMemcpyAsync(e->li_keep.p, keep, nkeep, hipMemcpyHostToDevice, st));
    return CSS_OK;
}

// What the sparse entry points need of the encoder: BERT and a masked-LM head.
int check_sparse_state(const css_encoder* e, const char* fn) {
    CSS_REQUIRE(e->cfg.arch == CSS_ENCODER_ARCH_BERT, "%s: the encoder is not a BERT model (the masked-LM head exists for "
                "arch = BERT only)", fn);
    if (!e->mlm_set) {
        css::set_error("%s: no masked-LM head (call css_encoder_set_mlm_head first)", fn);
        return CSS_ERR_STATE;
    }
    return CSS_OK;
}

// g_t = LayerNorm(gelu(Wd h_t + bd)) over the rows that the forward just enqueued on `st` left behind: fp32 rows into
// g32 and, in bf16 mode, their one rounding into g16.  Unfolded paths: the fp32 GEMM over x32 (both modes; u in qkv).
// LayerNorm-folded path: x32 does not exist, so k_tok_vec_ln finishes the last LayerNorm into bf16 rows (ctx), the bf16
// GEMM forms u (qkv), and g16 may be ctx again (the GEMM has read it by then).
int mlm_rows(css_encoder* e, int T, float* g32, bf16_t* g16, hipStream_t st) {
    const css_encoder_cfg& c = e->cfg;
    const int H = c.hidden;
    const float *W = e->mlm_w.p, *bd = W + (size_t)H * H, *lg = bd + H, *lb = lg + H;
    int rc;
    const dim3 grid((T + 3) / 4), blk(256);
    if (!e->x32_valid) {
        const LayerW& L = e->layers.back();
        {
            ProfScope ps("enc_mlm_rows", st);
            hipLaunchKernelGGL(k_tok_vec_ln<768>, dim3((T + 15) / 16), blk, 0, st, (const bf16_t*)e->x16, e->stats[0], L.ln2g,
                               L.ln2b, 1.0f / H, c.ln_eps, T, (const float*)nullptr, H, 0, (bf16_t*)e->ctx);
            CSS_LAUNCH_CHECK();
        }
        if ((rc = launch_gemm<bf16_t, EPI_GELU>(e->ctx, e->mlm_wd16.p, bd, e->qkv, T, H, H, 0, 1.0f, e->num_cus, st,
                                                "enc_mlm_dense")) != CSS_OK)
            return rc;
        ProfScope ps("enc_mlm_ln", st);
        hipLaunchKernelGGL((k_mlm_ln<768, bf16_t>), grid, blk, 0, st, (const bf16_t*)e->qkv, lg, lb, c.ln_eps, g32, g16, T);
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    if ((rc = launch_gemm<float, EPI_GELU>(e->x32, W, bd, e->qkv, T, H, H, 0, 1.0f, e->num_cus, st, "enc_mlm_dense")) != CSS_OK)
        return rc;
    ProfScope ps("enc_mlm_ln", st);
    if (H == 384) hipLaunchKernelGGL((k_mlm_ln<384, float>), grid, blk, 0, st, (const float*)e->qkv, lg, lb, c.ln_eps, g32, g16, T);
    else hipLaunchKernelGGL((k_mlm_ln<768, float>), grid, blk, 0, st, (const float*)e->qkv, lg, lb, c.ln_eps, g32, g16, T);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// zmax [B][V] (bit patterns) of the token rows `rows` ([T][H], bf16 in bf16 mode, fp32 in fp32 mode): zero fill, then
// k_vocab_max.  The fill makes every call start from nothing, whatever an earlier call left in the buffer.
int launch_vocab_max(css_encoder* e, const void* rows, const int32_t* cu, int B, int T, unsigned* zmax, hipStream_t st) {
    const css_encoder_cfg& c = e->cfg;
    CSS_HIP_TRY(hipMemsetAsync(zmax, 0, (size_t)B * c.vocab * 4, st));
    ProfScope ps("enc_vocab_max", st);
    const dim3 grid((c.vocab + 127) / 128, (T + 127) / 128), blk(256);
    if (c.compute == 0)
        hipLaunchKernelGGL(k_vocab_max<bf16_t>, grid, blk, 0, st, (const bf16_t*)rows, cu, B, T, (const bf16_t*)e->mlm_e16.p,
                           (const float*)e->mlm_c.p, c.vocab, c.hidden, zmax);
    else
        hipLaunchKernelGGL(k_vocab_max<float>, grid, blk, 0, st, (const float*)rows, cu, B, T, e->mlm_e32, (const float*)e->mlm_c.p,
                           c.vocab, c.hidden, zmax);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Forward, head, vocabulary maximum and top-m on `st`.  g32: where the fp32 rows g go (the caller's rows_out, or
// pre32, which is free after the forward); zmax: the caller's dense_out or sp_z.
int forward_sparse_any(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int T, int max_len, int m, int32_t* terms,
                       float* weights, int32_t* nnz, unsigned* zmax, float* g32, hipStream_t st) {
    int rc = forward_any(e, ids, cu, B, T, max_len, 0, e->out_dev, st);
    if (rc != CSS_OK) return rc;
    const bool bf = e->cfg.compute == 0;
    if ((rc = mlm_rows(e, T, g32, bf ? (bf16_t*)e->ctx : nullptr, st)) != CSS_OK) return rc;
    if ((rc = launch_vocab_max(e, bf ? (const void*)e->ctx : (const void*)g32, cu, B, T, zmax, st)) != CSS_OK) return rc;
    ProfScope ps("enc_vocab_topm", st);
    hipLaunchKernelGGL(k_vocab_topm, dim3(B), dim3(256), 0, st, (const unsigned*)zmax, e->cfg.vocab, m, terms, weights, nnz);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

}  // namespace

extern "C" {

int css_encoder_create(const css_encoder_cfg* cfg, int device, css_encoder** out) {
    CSS_REQUIRE(cfg && out, "css_encoder_create: NULL argument");
    CSS_REQUIRE(cfg->arch == CSS_ENCODER_ARCH_MPNET || cfg->arch == CSS_ENCODER_ARCH_BERT,
                "css_encoder_create: arch must be 0 (MPNet) or 1 (BERT) (got %d)", cfg->arch);
    CSS_REQUIRE(cfg->pooling == CSS_ENCODER_POOL_MEAN || cfg->pooling == CSS_ENCODER_POOL_CLS,
                "css_encoder_create: pooling must be 0 (mean) or 1 (CLS) (got %d)", cfg->pooling);
    const bool bert = cfg->arch == CSS_ENCODER_ARCH_BERT;
    if (bert)
        CSS_REQUIRE((cfg->hidden == 384 || cfg->hidden == 768) && cfg->heads >= 1 && cfg->hidden % cfg->heads == 0 &&
                        (cfg->hidden / cfg->heads == 32 || cfg->hidden / cfg->heads == 64),
                    "css_encoder_create: BERT kernels are built for hidden 384 / 768 with head_dim 32 / 64 (got hidden=%d "
                    "heads=%d)", cfg->hidden, cfg->heads);
    else
        CSS_REQUIRE(cfg->hidden == 768 && cfg->heads * 64 == cfg->hidden,
                    "css_encoder_create: kernels are built for hidden=768, head_dim=64 (got hidden=%d heads=%d)", cfg->hidden,
                    cfg->heads);
    CSS_REQUIRE(cfg->ffn % 128 == 0 && cfg->ffn >= 128, "css_encoder_create: ffn must be a multiple of 128");
    CSS_REQUIRE(cfg->num_layers >= 1 && cfg->num_layers <= 64, "css_encoder_create: num_layers out of range");
    CSS_REQUIRE(cfg->max_seq_len >= 1 && cfg->max_seq_len <= 512, "css_encoder_create: max_seq_len outside [1, 512]");
    CSS_REQUIRE(cfg->max_pos >= cfg->max_seq_len + pos_offset(*cfg), "css_encoder_create: max_pos must be >= max_seq_len + %d",
                pos_offset(*cfg));
    // (a vocabulary of one row, the pad id, runs no forward pass, and css_encoder_vocab_max needs none)
    CSS_REQUIRE(cfg->vocab >= 1 && (bert || (cfg->rel_buckets >= 4 && cfg->rel_buckets % 4 == 0)),
                "css_encoder_create: bad vocab / rel_buckets");
    CSS_REQUIRE(cfg->pad_id >= 0 && cfg->pad_id < cfg->vocab, "css_encoder_create: pad_id outside the vocabulary");
    CSS_REQUIRE(cfg->compute == 0 || cfg->compute == 1, "css_encoder_create: compute must be 0 (bf16) or 1 (fp32)");
    int rc = css::check_device(device);
    if (rc != CSS_OK) return rc;
    DeviceGuard g(device);
    css_encoder* e = new css_encoder();
    e->cfg = *cfg;
    e->device = device;
    {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, device) == hipSuccess) e->num_cus = p.multiProcessorCount;
    }
    hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (err != hipSuccess) {
        delete e;
        return css::hip_fail(err, "hipStreamCreate", __FILE__, __LINE__);
    }
    rc = build_params(e);
    if (rc != CSS_OK) {
        css_encoder_free(e);
        return rc;
    }
    *out = e;
    return CSS_OK;
}

int css_encoder_free(css_encoder* e) {
    if (!e) return CSS_OK;
    DeviceGuard g(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& kv : e->graphs)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    for (auto& kv : e->params)   // q/k/v views alias the fused tensors: free only owning entries
        if (kv.second.owned && kv.second.p) (void)hipFree(kv.second.p);
    for (void* p : e->extra)
        if (p) (void)hipFree(p);
    for (auto& L : e->layers) {
        if (L.wqkv_h) (void)hipFree(L.wqkv_h);
        if (L.wo_h) (void)hipFree(L.wo_h);
        if (L.w1_h) (void)hipFree(L.w1_h);
        if (L.w2_h) (void)hipFree(L.w2_h);
        void* fp[] = {L.wqkv_f, L.w1_f, L.w2_p, L.wo_p, L.dqkv, L.d1, L.bo_f, L.b2_f};
        for (void* p : fp)
            if (p) (void)hipFree(p);
    }
    void* ptrs[] = {e->bias_tab, e->bucket_dev, e->x32, e->pre32, e->x16, e->qkv, e->ctx, e->ffn, e->ids_dev,
                    e->cu_dev, e->out_dev, e->stats[0], e->stats[1], e->spans_dev, e->span_out_dev, e->span_scores_dev,
                    e->span_q_dev, e->head_dev, e->seg_dev, e->logits_dev, e->tokw_dev};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return CSS_OK;
}

int css_encoder_load_weights(css_encoder* e, const css_tensor* tensors, int n) {
    CSS_REQUIRE(e && tensors && n >= 0, "css_encoder_load_weights: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    // A checkpoint must cover every parameter exactly once: a missing tensor would leave uninitialised device
    // memory in the model, a duplicate (the same key under two prefixes) makes the result depend on the order.
    std::map<std::string, int> seen;
    for (int i = 0; i < n; ++i) {
        CSS_REQUIRE(tensors[i].name && tensors[i].data, "css_encoder_load_weights: tensor %d has NULL name/data", i);
        std::string name = tensors[i].name;
        const std::string pfx = "0.auto_model.";  // sentence-transformers module prefix
        if (name.compare(0, pfx.size(), pfx) == 0) name = name.substr(pfx.size());
        const bool bert = e->cfg.arch == CSS_ENCODER_ARCH_BERT;
        const std::string apfx = bert ? "bert." : "mpnet.";   // the architecture's own model prefix
        if (name.compare(0, apfx.size(), apfx) == 0) name = name.substr(apfx.size());
        if (name.compare(0, 7, "pooler.") == 0 || name == "embeddings.position_ids") continue;  // unused
        if (bert && name == "embeddings.token_type_ids") continue;   // (a buffer of BertEmbeddings)
        auto it = e->params.find(name);
        CSS_REQUIRE(it != e->params.end(), "css_encoder_load_weights: unknown parameter '%s'", name.c_str());
        CSS_REQUIRE(it->second.numel == tensors[i].numel, "css_encoder_load_weights: '%s' has %lld elements, expected %lld",
                    name.c_str(), (long long)tensors[i].numel, (long long)it->second.numel);
        CSS_REQUIRE(seen[name]++ == 0, "css_encoder_load_weights: parameter '%s' appears more than once", name.c_str());
        CSS_HIP_TRY(hipMemcpy(it->second.p, tensors[i].data, (size_t)tensors[i].numel * 4, hipMemcpyHostToDevice));
    }
    for (const auto& kv : e->params) {
        const std::string& nm = kv.first;
        const bool view = !kv.second.required;
        const size_t fq = nm.find(".attn.qkv.");
        if (fq != std::string::npos) {
            // fused [3H, H] weight / [3H] bias: given as one tensor, or as its three HF views q, k, v -- not both
            int parts = 0;
            for (const char* v : {"q", "k", "v"}) {
                std::string vn = nm;
                vn.replace(fq, 10, std::string(".attn.") + v + ".");
                parts += seen.count(vn) ? 1 : 0;
            }
            const bool whole = seen.count(nm) != 0;
            CSS_REQUIRE(!(whole && parts > 0), "css_encoder_load_weights: '%s' given both fused and as q/k/v", nm.c_str());
            CSS_REQUIRE(whole || parts == 3, "css_encoder_load_weights: checkpoint does not cover '%s' (q/k/v: %d of 3)",
                        nm.c_str(), parts);
        } else if (!view) {
            CSS_REQUIRE(seen.count(nm) != 0, "css_encoder_load_weights: checkpoint has no tensor for '%s'", nm.c_str());
        }
    }
    return finalize_weights(e);
}

int css_encoder_init_synthetic(css_encoder* e, uint64_t seed) {
    CSS_REQUIRE(e, "css_encoder_init_synthetic: NULL encoder");
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    for (auto& kv : e->params) {
        if (!kv.second.synth) continue;   // (MPNet q/k/v views: the fused tensor is filled)
        const Param& p = kv.second;
        hipLaunchKernelGGL(k_synth_fill, dim3(1024), dim3(256), 0, e->stream, p.p, (size_t)p.numel,
                           css_synth_tensor_seed(seed, p.synth_id), p.mean, p.std);
    }
    // padding_idx rows are zero at init (word_embeddings[pad], and for MPNet position_embeddings[pad]; BERT's position
    // table has no padding row)
    const int H = e->cfg.hidden;
    hipLaunchKernelGGL(k_zero_row, dim3((H + 255) / 256), dim3(256), 0, e->stream, e->wemb + (size_t)e->cfg.pad_id * H, H);
    if (e->cfg.arch != CSS_ENCODER_ARCH_BERT)
        hipLaunchKernelGGL(k_zero_row, dim3((H + 255) / 256), dim3(256), 0, e->stream, e->pemb + (size_t)e->cfg.pad_id * H, H);
    CSS_LAUNCH_CHECK();
    return finalize_weights(e);
}

int css_encoder_export_weight(const css_encoder* ce, const char* name, float* out_host, int64_t numel) {
    css_encoder* e = const_cast<css_encoder*>(ce);
    CSS_REQUIRE(e && name && out_host, "css_encoder_export_weight: NULL argument");
    auto it = e->params.find(name);
    CSS_REQUIRE(it != e->params.end(), "css_encoder_export_weight: unknown parameter '%s'", name);
    CSS_REQUIRE(it->second.numel == numel, "css_encoder_export_weight: '%s' has %lld elements, not %lld", name,
                (long long)it->second.numel, (long long)numel);
    DeviceGuard g(e->device);
    CSS_HIP_TRY(hipMemcpy(out_host, it->second.p, (size_t)numel * 4, hipMemcpyDeviceToHost));
    return CSS_OK;
}

int css_encoder_set_attention_range(css_encoder* e, float range) {
    CSS_REQUIRE(e, "css_encoder_set_attention_range: NULL encoder");
    CSS_REQUIRE(range == 0.f || (range >= 1.f && range <= 1.2676506e30f), "css_encoder_set_attention_range: range must be 0 or in [1, 2^100]");
    std::lock_guard<std::mutex> lk(e->mu);
    e->att_range = range;
    // captured tiny-batch graphs hold the old kernel argument
    for (auto& kv : e->graphs)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    e->graphs.clear();
    return CSS_OK;
}

int css_encoder_debug_read(css_encoder* e, const char* what, float* out_host, int64_t numel) {
    CSS_REQUIRE(e && what && out_host && numel > 0, "css_encoder_debug_read: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    const std::string w = what;
    const bool bf = e->cfg.compute == 0;
    const void* src = nullptr;
    bool typed = true;  // operand-typed (bf16 in product mode) vs always fp32
    if (w == "x32") {
        CSS_REQUIRE(e->x32_valid, "css_encoder_debug_read: the last forward ran the LayerNorm-folded path, which does not "
                                  "materialise x32");
        src = e->x32;
        typed = false;
    }
    else if (w == "pre32") { src = e->pre32; typed = false; }
    else if (w == "qkv") src = e->qkv;
    else if (w == "ctx") src = e->ctx;
    else if (w == "ffn") src = e->ffn;
    CSS_REQUIRE(src != nullptr, "css_encoder_debug_read: unknown or unallocated buffer '%s'", what);
    CSS_HIP_TRY(hipDeviceSynchronize());
    if (typed && bf) {
        std::vector<uint16_t> tmp((size_t)numel);
        CSS_HIP_TRY(hipMemcpy(tmp.data(), src, (size_t)numel * 2, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < numel; ++i) {
            const uint32_t u = (uint32_t)tmp[i] << 16;
            memcpy(&out_host[i], &u, 4);
        }
    } else {
        CSS_HIP_TRY(hipMemcpy(out_host, src, (size_t)numel * 4, hipMemcpyDeviceToHost));
    }
    return CSS_OK;
}

int css_encoder_forward(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int normalize, float* out) {
    CSS_REQUIRE(e && ids && cu && out, "css_encoder_forward: NULL argument");
    int max_len = 0;
    int rc = check_batch(e, ids, cu, B, &max_len);
    if (rc != CSS_OK) return rc;
    const int T = cu[B];
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    rc = ensure_acts(e, T, B);
    if (rc != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(e->ids_dev, ids, (size_t)T * 4, hipMemcpyHostToDevice, e->stream));
    CSS_HIP_TRY(hipMemcpyAsync(e->cu_dev, cu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, e->stream));
    bool done = false;
    if (e->graphs_ok && T <= 64 && B <= 8 && !css::prof_enabled()) {
        // ~90 launches of a few microseconds each: replay them as one hipGraph
        const uint64_t key = ((uint64_t)B << 40) | ((uint64_t)T << 20) | ((uint64_t)max_len << 1) | (normalize ? 1u : 0u);
        auto& ge = e->graphs[key];
        ++ge.uses;
        if (ge.exec == nullptr && ge.uses == 2) {
            hipGraph_t graph = nullptr;
            if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int frc = forward_any(e, e->ids_dev, e->cu_dev, B, T, max_len, normalize, e->out_dev, e->stream);
                const hipError_t ce = hipStreamEndCapture(e->stream, &graph);
                if (frc == CSS_OK && ce == hipSuccess && graph &&
                    hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                    // instantiated
                } else {
                    ge.exec = nullptr;
                    e->graphs_ok = false;  // fall back to eager launches for good
                    (void)hipGetLastError();
                }
                if (graph) (void)hipGraphDestroy(graph);
            } else {
                e->graphs_ok = false;
                (void)hipGetLastError();
            }
        }
        if (ge.exec) {
            CSS_HIP_TRY(hipGraphLaunch(ge.exec, e->stream));
            done = true;
        }
    }
    if (!done && (rc = forward_any(e, e->ids_dev, e->cu_dev, B, T, max_len, normalize, e->out_dev, e->stream)) != CSS_OK)
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(out, e->out_dev, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, e->stream));
    CSS_HIP_TRY(hipStreamSynchronize(e->stream));
    return CSS_OK;
}

int css_encoder_forward_dev(css_encoder* e, const int32_t* ids_dev, const int32_t* cu_dev, int B, int total_tokens,
                            int max_len, int normalize, float* out_dev, void* stream) {
    CSS_REQUIRE(e && ids_dev && cu_dev && out_dev, "css_encoder_forward_dev: NULL argument");
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    int rc = ensure_acts(e, total_tokens, B);
    if (rc != CSS_OK) return rc;
    return forward_any(e, ids_dev, cu_dev, B, total_tokens, max_len, normalize, out_dev, (hipStream_t)stream);
}

int css_encoder_forward_spans(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, const int32_t* spans, int S,
                              const float* q, int normalize, float* seq_out, float* span_out, float* scores_out) {
    CSS_REQUIRE(e && ids && cu, "css_encoder_forward_spans: NULL argument");
    CSS_REQUIRE(S >= 0 && (S == 0 || spans), "css_encoder_forward_spans: S=%d is negative, or spans is NULL", S);
    CSS_REQUIRE((q != nullptr) == (scores_out != nullptr), "css_encoder_forward_spans: q and scores_out go together");
    int max_len = 0;
    int rc = check_batch(e, ids, cu, B, &max_len);
    if (rc != CSS_OK) return rc;
    for (int s = 0; s < S; ++s) {
        const int b = spans[3 * s], lo = spans[3 * s + 1], hi = spans[3 * s + 2];
        CSS_REQUIRE(b >= 0 && b < B, "css_encoder_forward_spans: span %d names sequence %d outside [0, %d)", s, b, B);
        const int len = cu[b + 1] - cu[b];
        CSS_REQUIRE(lo >= 0 && lo < hi && hi <= len,
                    "css_encoder_forward_spans: span %d is [%d, %d) of sequence %d: need 0 <= begin < end <= %d", s, lo, hi, b, len);
    }
    const int T = cu[B];
    const size_t H = e->cfg.hidden;
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    if ((rc = ensure_acts(e, T, B)) != CSS_OK || (rc = ensure_spans(e, S)) != CSS_OK) return rc;
    hipStream_t st = e->stream;
    CSS_HIP_TRY(hipMemcpyAsync(e->ids_dev, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->cu_dev, cu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
    if (S) CSS_HIP_TRY(hipMemcpyAsync(e->spans_dev, spans, (size_t)S * 12, hipMemcpyHostToDevice, st));
    if (q) CSS_HIP_TRY(hipMemcpyAsync(e->span_q_dev, q, H * 4, hipMemcpyHostToDevice, st));
    // eager launches (the tiny-batch graphs replay css_encoder_forward only)
    if ((rc = forward_any(e, e->ids_dev, e->cu_dev, B, T, max_len, normalize, e->out_dev, st)) != CSS_OK) return rc;
    if ((rc = pool_spans(e, e->cu_dev, B, e->spans_dev, S, q ? e->span_q_dev : nullptr, normalize,
                         span_out ? e->span_out_dev : nullptr, scores_out ? e->span_scores_dev : nullptr, st)) != CSS_OK)
        return rc;
    if (seq_out) CSS_HIP_TRY(hipMemcpyAsync(seq_out, e->out_dev, (size_t)B * H * 4, hipMemcpyDeviceToHost, st));
    if (span_out && S) CSS_HIP_TRY(hipMemcpyAsync(span_out, e->span_out_dev, (size_t)S * H * 4, hipMemcpyDeviceToHost, st));
    if (scores_out && S) CSS_HIP_TRY(hipMemcpyAsync(scores_out, e->span_scores_dev, (size_t)S * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_forward_spans_dev(css_encoder* e, const int32_t* ids_dev, const int32_t* cu_dev, int B, int total_tokens,
                                  int max_len, const int32_t* spans_dev, int S, const float* q_dev, int normalize,
                                  float* seq_out_dev, float* span_out_dev, float* scores_out_dev, void* stream) {
    CSS_REQUIRE(e && ids_dev && cu_dev, "css_encoder_forward_spans_dev: NULL argument");
    CSS_REQUIRE(S >= 0 && (S == 0 || spans_dev), "css_encoder_forward_spans_dev: S=%d is negative, or spans is NULL", S);
    CSS_REQUIRE((q_dev != nullptr) == (scores_out_dev != nullptr), "css_encoder_forward_spans_dev: q and scores_out go together");
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    int rc = ensure_acts(e, total_tokens, B);
    if (rc != CSS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    // (seq_out NULL: the sequence rows go to the encoder's own buffer)
    if ((rc = forward_any(e, ids_dev, cu_dev, B, total_tokens, max_len, normalize, seq_out_dev ? seq_out_dev : e->out_dev, st)) != CSS_OK)
        return rc;
    return pool_spans(e, cu_dev, B, spans_dev, S, q_dev, normalize, span_out_dev, scores_out_dev, st);
}

int css_encoder_set_head(css_encoder* e, const float* pooler_w, const float* pooler_b, const float* cls_w, const float* cls_b) {
    CSS_REQUIRE(e && pooler_w && pooler_b && cls_w && cls_b, "css_encoder_set_head: NULL argument");
    CSS_REQUIRE(e->cfg.arch == CSS_ENCODER_ARCH_BERT, "css_encoder_set_head: the encoder is not a BERT model (the "
                "classification head exists for arch = BERT only)");
    const size_t H = e->cfg.hidden;
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    if (!e->head_dev) CSS_HIP_TRY(hipMalloc((void**)&e->head_dev, (H * H + 2 * H + 1) * 4));
    e->head_set = false;   // (a failed copy leaves no half-replaced head in use)
    // the stream is idle between calls (every host entry point ends with a synchronise)
    CSS_HIP_TRY(hipMemcpy(e->head_dev, pooler_w, H * H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(e->head_dev + H * H, pooler_b, H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(e->head_dev + H * H + H, cls_w, H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(e->head_dev + H * H + 2 * H, cls_b, 4, hipMemcpyHostToDevice));
    e->head_set = true;
    return CSS_OK;
}

int css_encoder_forward_pairs(css_encoder* e, const int32_t* ids, const int32_t* cu, const int32_t* seg_starts, int B,
                              float* logits_out) {
    CSS_REQUIRE(e && ids && cu && seg_starts && logits_out, "css_encoder_forward_pairs: NULL argument");
    int max_len = 0;
    int rc = check_batch(e, ids, cu, B, &max_len);
    if (rc != CSS_OK) return rc;
    for (int b = 0; b < B; ++b) {
        const int len = cu[b + 1] - cu[b];
        CSS_REQUIRE(seg_starts[b] >= 1 && seg_starts[b] <= len,
                    "css_encoder_forward_pairs: sequence %d has seg_start %d outside [1, %d]", b, seg_starts[b], len);
    }
    const int T = cu[B];
    std::lock_guard<std::mutex> lk(e->mu);
    if ((rc = check_pairs_state(e, "css_encoder_forward_pairs")) != CSS_OK) return rc;
    DeviceGuard g(e->device);
    if ((rc = ensure_acts(e, T, B)) != CSS_OK || (rc = ensure_pairs(e, B)) != CSS_OK) return rc;
    hipStream_t st = e->stream;
    CSS_HIP_TRY(hipMemcpyAsync(e->ids_dev, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->cu_dev, cu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->seg_dev, seg_starts, (size_t)B * 4, hipMemcpyHostToDevice, st));
    // eager launches (the tiny-batch graphs replay css_encoder_forward only)
    if ((rc = forward_pairs_any(e, e->ids_dev, e->cu_dev, e->seg_dev, B, T, max_len, e->logits_dev, st)) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(logits_out, e->logits_dev, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_forward_pairs_dev(css_encoder* e, const int32_t* ids_dev, const int32_t* cu_dev, const int32_t* seg_starts_dev,
                                  int B, int total_tokens, int max_len, float* logits_out_dev, void* stream) {
    CSS_REQUIRE(e && ids_dev && cu_dev && seg_starts_dev && logits_out_dev, "css_encoder_forward_pairs_dev: NULL argument");
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_pairs_state(e, "css_encoder_forward_pairs_dev");
    if (rc != CSS_OK) return rc;
    DeviceGuard g(e->device);
    if ((rc = ensure_acts(e, total_tokens, B)) != CSS_OK) return rc;
    return forward_pairs_any(e, ids_dev, cu_dev, seg_starts_dev, B, total_tokens, max_len, logits_out_dev, (hipStream_t)stream);
}

int css_encoder_set_token_projection(css_encoder* e, const float* W, int P) {
    CSS_REQUIRE(e, "css_encoder_set_token_projection: NULL argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!W) {
        e->tok_p = 0;
        return CSS_OK;
    }
    CSS_REQUIRE(P % 32 == 0 && P >= 32 && P <= kTokMaxP,
                "css_encoder_set_token_projection: P=%d must be a multiple of 32 in [32, %d]", P, kTokMaxP);
    const size_t H = e->cfg.hidden;
    DeviceGuard g(e->device);
    if (!e->tokw_dev) CSS_HIP_TRY(hipMalloc((void**)&e->tokw_dev, (size_t)kTokMaxP * H * 4));
    e->tok_p = 0;   // (a failed copy leaves no half-replaced projection in use)
    // the stream is idle between calls (every host entry point ends with a synchronise)
    CSS_HIP_TRY(hipMemcpy(e->tokw_dev, W, (size_t)P * H * 4, hipMemcpyHostToDevice));
    e->tok_p = P;
    return CSS_OK;
}

int css_encoder_token_dim(css_encoder* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    return token_dim(e);
}

int css_encoder_forward_tokens(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int normalize, uint16_t* tok_out,
                               float* seq_out) {
    CSS_REQUIRE(e && ids && cu && tok_out, "css_encoder_forward_tokens: NULL argument");
    int max_len = 0;
    int rc = check_batch(e, ids, cu, B, &max_len);
    if (rc != CSS_OK) return rc;
    const int T = cu[B];
    const size_t H = e->cfg.hidden;
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    const size_t P = token_dim(e);
    if ((rc = ensure_acts(e, T, B)) != CSS_OK || (rc = e->li_tok.grow((size_t)T * P)) != CSS_OK) return rc;
    hipStream_t st = e->stream;
    CSS_HIP_TRY(hipMemcpyAsync(e->ids_dev, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->cu_dev, cu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
    // eager launches (the tiny-batch graphs replay css_encoder_forward only)
    if ((rc = forward_any(e, e->ids_dev, e->cu_dev, B, T, max_len, normalize, e->out_dev, st)) != CSS_OK) return rc;
    if ((rc = write_tokens(e, T, normalize, e->li_tok.p, st)) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(tok_out, e->li_tok.p, (size_t)T * P * 2, hipMemcpyDeviceToHost, st));
    if (seq_out) CSS_HIP_TRY(hipMemcpyAsync(seq_out, e->out_dev, (size_t)B * H * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_forward_tokens_dev(css_encoder* e, const int32_t* ids_dev, const int32_t* cu_dev, int B, int total_tokens,
                                   int max_len, int normalize, uint16_t* tok_out_dev, float* seq_out_dev, void* stream) {
    CSS_REQUIRE(e && ids_dev && cu_dev && tok_out_dev, "css_encoder_forward_tokens_dev: NULL argument");
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    int rc = ensure_acts(e, total_tokens, B);
    if (rc != CSS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    // (seq_out NULL: the sequence rows go to the encoder's own buffer)
    if ((rc = forward_any(e, ids_dev, cu_dev, B, total_tokens, max_len, normalize, seq_out_dev ? seq_out_dev : e->out_dev, st)) != CSS_OK)
        return rc;
    return write_tokens(e, total_tokens, normalize, tok_out_dev, st);
}

int css_encoder_maxsim(css_encoder* e, const uint16_t* q_tok, const int32_t* cu_q, int nq, const uint16_t* d_tok,
                       const int32_t* cu_d, int nd, const uint8_t* d_keep, const int32_t* pairs, int np, int P,
                       float* scores_out) {
    CSS_REQUIRE(e && q_tok && cu_q && d_tok && cu_d && (scores_out || np == 0), "css_encoder_maxsim: NULL argument");
    CSS_REQUIRE(maxsim_width_ok(P), "css_encoder_maxsim: P=%d must be a multiple of 32 in [32, 128], or 384, or 768", P);
    int rc = check_maxsim("css_encoder_maxsim", cu_q, nq, cu_d, nd, d_keep, pairs, np);
    if (rc != CSS_OK) return rc;
    if (np == 0) return CSS_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    const size_t ndt = (size_t)cu_d[nd];
    if ((rc = e->li_tok.grow(ndt * P)) != CSS_OK || (rc = e->li_cud.grow((size_t)nd + 1)) != CSS_OK ||
        (rc = upload_maxsim(e, q_tok, cu_q, nq, d_keep, ndt, pairs, np, P, st)) != CSS_OK)
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(e->li_tok.p, d_tok, ndt * P * 2, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->li_cud.p, cu_d, ((size_t)nd + 1) * 4, hipMemcpyHostToDevice, st));
    if ((rc = launch_maxsim(e, e->li_q.p, e->li_cuq.p, nq, e->li_tok.p, e->li_cud.p, nd, d_keep ? e->li_keep.p : nullptr,
                            e->li_pairs.p, np, P, e->li_scores.p, st)) != CSS_OK)
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(scores_out, e->li_scores.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_maxsim_dev(css_encoder* e, const uint16_t* q_tok_dev, const int32_t* cu_q_dev, int nq, const uint16_t* d_tok_dev,
                           const int32_t* cu_d_dev, int nd, const uint8_t* d_keep_dev, const int32_t* pairs_dev, int np, int P,
                           float* scores_out_dev, void* stream) {
    CSS_REQUIRE(e && q_tok_dev && cu_q_dev && d_tok_dev && cu_d_dev && (np == 0 || (pairs_dev && scores_out_dev)),
                "css_encoder_maxsim_dev: NULL argument");
    CSS_REQUIRE(maxsim_width_ok(P), "css_encoder_maxsim_dev: P=%d must be a multiple of 32 in [32, 128], or 384, or 768", P);
    CSS_REQUIRE(nq >= 1 && nd >= 1 && np >= 0, "css_encoder_maxsim_dev: need nq >= 1, nd >= 1, np >= 0 (got %d, %d, %d)", nq, nd, np);
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    return launch_maxsim(e, q_tok_dev, cu_q_dev, nq, d_tok_dev, cu_d_dev, nd, d_keep_dev, pairs_dev, np, P, scores_out_dev,
                         (hipStream_t)stream);
}

int css_encoder_forward_maxsim(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, const uint16_t* q_tok,
                               const int32_t* cu_q, int nq, const uint8_t* d_keep, const int32_t* pairs, int np,
                               float* scores_out, uint16_t* tok_out) {
    CSS_REQUIRE(e && ids && cu && q_tok && cu_q && (scores_out || np == 0), "css_encoder_forward_maxsim: NULL argument");
    int max_len = 0;
    int rc = check_batch(e, ids, cu, B, &max_len);
    if (rc != CSS_OK) return rc;
    if ((rc = check_maxsim("css_encoder_forward_maxsim", cu_q, nq, cu, B, d_keep, pairs, np)) != CSS_OK) return rc;
    const int T = cu[B];
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    const int P = token_dim(e);
    hipStream_t st = e->stream;
    if ((rc = ensure_acts(e, T, B)) != CSS_OK || (rc = e->li_tok.grow((size_t)T * P)) != CSS_OK ||
        (rc = upload_maxsim(e, q_tok, cu_q, nq, d_keep, (size_t)T, pairs, np, P, st)) != CSS_OK)
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(e->ids_dev, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->cu_dev, cu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
    // eager launches (the tiny-batch graphs replay css_encoder_forward only)
    if ((rc = forward_any(e, e->ids_dev, e->cu_dev, B, T, max_len, 1, e->out_dev, st)) != CSS_OK) return rc;
    if ((rc = write_tokens(e, T, 1, e->li_tok.p, st)) != CSS_OK) return rc;
    if ((rc = launch_maxsim(e, e->li_q.p, e->li_cuq.p, nq, e->li_tok.p, e->cu_dev, B, d_keep ? e->li_keep.p : nullptr,
                            e->li_pairs.p, np, P, e->li_scores.p, st)) != CSS_OK)
        return rc;
    if (np) CSS_HIP_TRY(hipMemcpyAsync(scores_out, e->li_scores.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    if (tok_out) CSS_HIP_TRY(hipMemcpyAsync(tok_out, e->li_tok.p, (size_t)T * P * 2, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_forward_maxsim_dev(css_encoder* e, const int32_t* ids_dev, const int32_t* cu_dev, int B, int total_tokens,
                                   int max_len, const uint16_t* q_tok_dev, const int32_t* cu_q_dev, int nq,
                                   const uint8_t* d_keep_dev, const int32_t* pairs_dev, int np, float* scores_out_dev,
                                   uint16_t* tok_out_dev, void* stream) {
    CSS_REQUIRE(e && ids_dev && cu_dev && q_tok_dev && cu_q_dev && (np == 0 || (pairs_dev && scores_out_dev)),
                "css_encoder_forward_maxsim_dev: NULL argument");
    CSS_REQUIRE(nq >= 1 && np >= 0, "css_encoder_forward_maxsim_dev: need nq >= 1, np >= 0 (got %d, %d)", nq, np);
    std::lock_guard<std::mutex> lk(e->mu);
    DeviceGuard g(e->device);
    const int P = token_dim(e);
    int rc = ensure_acts(e, total_tokens, B);
    // (tok_out NULL: the token rows stay in the encoder's own buffer; growing it frees the old one, so work that an
    // earlier call enqueued on another stream must have finished, as for the activations)
    if (rc == CSS_OK && !tok_out_dev) rc = e->li_tok.grow((size_t)total_tokens * P);
    if (rc != CSS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    bf16_t* tok = tok_out_dev ? tok_out_dev : e->li_tok.p;
    if ((rc = forward_any(e, ids_dev, cu_dev, B, total_tokens, max_len, 1, e->out_dev, st)) != CSS_OK) return rc;
    if ((rc = write_tokens(e, total_tokens, 1, tok, st)) != CSS_OK) return rc;
    return launch_maxsim(e, q_tok_dev, cu_q_dev, nq, tok, cu_dev, B, d_keep_dev, pairs_dev, np, P, scores_out_dev, st);
}

int css_encoder_set_mlm_head(css_encoder* e, const float* dense_w, const float* dense_b, const float* ln_g, const float* ln_b,
                             const float* decoder_w, const float* decoder_b) {
    CSS_REQUIRE(e && dense_w && dense_b && ln_g && ln_b && decoder_b, "css_encoder_set_mlm_head: NULL argument");
    CSS_REQUIRE(e->cfg.arch == CSS_ENCODER_ARCH_BERT, "css_encoder_set_mlm_head: the encoder is not a BERT model (the "
                "masked-LM head exists for arch = BERT only)");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!decoder_w && !e->weights_ready) {
        css::set_error("css_encoder_set_mlm_head: a tied decoder (decoder_w == NULL) needs the word embeddings: load the "
                       "weights first");
        return CSS_ERR_STATE;
    }
    DeviceGuard g(e->device);
    const size_t H = e->cfg.hidden, V = e->cfg.vocab;
    const bool bf = e->cfg.compute == 0;
    int rc;
    css::DevBuf<float> tmp;       // bf16 mode, untied: the fp32 decoder lives until its bf16 copy is made
    css::DevBuf<float>& own = bf ? tmp : e->mlm_e32_own;   // where an untied fp32 decoder goes
    // every allocation first: a refusal here leaves the current head in place (the buffers have one size per encoder, so
    // a head that is in use is never reallocated)
    if ((rc = e->mlm_w.grow_exact(H * H + 3 * H, "hipMalloc(mlm head)")) != CSS_OK ||
        (rc = e->mlm_c.grow_exact(V, "hipMalloc(mlm head)")) != CSS_OK ||
        (bf && ((rc = e->mlm_wd16.grow_exact(H * H, "hipMalloc(mlm head)")) != CSS_OK ||
                (rc = e->mlm_e16.grow_exact(V * H, "hipMalloc(mlm decoder)")) != CSS_OK)) ||
        (decoder_w && (rc = own.grow_exact(V * H, "hipMalloc(mlm decoder)")) != CSS_OK))
        return rc;
    // nothing was refused: from here on the old head is being replaced (a failed copy leaves no head in use).  The
    // stream is idle between calls (every host entry point ends with a synchronise).
    e->mlm_set = false;
    float* w = e->mlm_w.p;
    CSS_HIP_TRY(hipMemcpy(w, dense_w, H * H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(w + H * H, dense_b, H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(w + H * H + H, ln_g, H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(w + H * H + 2 * H, ln_b, H * 4, hipMemcpyHostToDevice));
    CSS_HIP_TRY(hipMemcpy(e->mlm_c.p, decoder_b, V * 4, hipMemcpyHostToDevice));
    const float* e32 = e->wemb;   // tied: the word embeddings as they are now
    if (decoder_w) {
        CSS_HIP_TRY(hipMemcpy(own.p, decoder_w, V * H * 4, hipMemcpyHostToDevice));
        e32 = own.p;
    }
    if (bf) {
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, e->stream, w, e->mlm_wd16.p, H * H);
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, e->stream, e32, e->mlm_e16.p, V * H);
        CSS_LAUNCH_CHECK();
        CSS_HIP_TRY(hipStreamSynchronize(e->stream));
    }
    e->mlm_e32 = bf ? nullptr : e32;
    e->mlm_set = true;
    return CSS_OK;
}

int css_encoder_vocab_max(css_encoder* e, const float* rows, const int32_t* cu, int B, float* zmax_out) {
    CSS_REQUIRE(e && rows && cu && zmax_out, "css_encoder_vocab_max: NULL argument");
    CSS_REQUIRE(B >= 1, "css_encoder_vocab_max: B < 1");
    CSS_REQUIRE(cu[0] == 0, "css_encoder_vocab_max: cu_seqlens[0] must be 0");
    for (int b = 0; b < B; ++b)
        CSS_REQUIRE(cu[b + 1] - cu[b] >= 1, "css_encoder_vocab_max: sequence %d has length %d (need at least 1)", b,
                    cu[b + 1] - cu[b]);
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_sparse_state(e, "css_encoder_vocab_max");
    if (rc != CSS_OK) return rc;
    DeviceGuard g(e->device);
    const size_t T = (size_t)cu[B], H = e->cfg.hidden, V = e->cfg.vocab;
    const bool bf = e->cfg.compute == 0;
    if ((rc = e->sp_rows.grow(T * H)) != CSS_OK || (rc = e->sp_cu.grow((size_t)B + 1)) != CSS_OK ||
        (rc = e->sp_z.grow((size_t)B * V)) != CSS_OK || (bf && (rc = e->sp_g16.grow(T * H)) != CSS_OK))
        return rc;
    hipStream_t st = e->stream;
    CSS_HIP_TRY(hipMemcpyAsync(e->sp_rows.p, rows, T * H * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->sp_cu.p, cu, ((size_t)B + 1) * 4, hipMemcpyHostToDevice, st));
    if (bf) {
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, st, (const float*)e->sp_rows.p, e->sp_g16.p, T * H);
        CSS_LAUNCH_CHECK();
    }
    if ((rc = launch_vocab_max(e, bf ? (const void*)e->sp_g16.p : (const void*)e->sp_rows.p, e->sp_cu.p, B, (int)T, e->sp_z.p,
                               st)) != CSS_OK)
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(zmax_out, e->sp_z.p, (size_t)B * V * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_vocab_max_dev(css_encoder* e, const float* rows_dev, const int32_t* cu_dev, int B, int total_tokens,
                              float* zmax_out_dev, void* stream) {
    CSS_REQUIRE(e && rows_dev && cu_dev && zmax_out_dev, "css_encoder_vocab_max_dev: NULL argument");
    CSS_REQUIRE(B >= 1 && total_tokens >= B, "css_encoder_vocab_max_dev: bad batch (B=%d, tokens=%d)", B, total_tokens);
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_sparse_state(e, "css_encoder_vocab_max_dev");
    if (rc != CSS_OK) return rc;
    DeviceGuard g(e->device);
    hipStream_t st = (hipStream_t)stream;
    const void* rows = rows_dev;
    if (e->cfg.compute == 0) {
        // (the bf16 rounding of the rows lives in a buffer of the encoder's that only grows; growing frees the old one,
        // so work that an earlier call enqueued on another stream must have finished, as for the activations)
        const size_t n = (size_t)total_tokens * e->cfg.hidden;
        if ((rc = e->sp_g16.grow(n)) != CSS_OK) return rc;
        hipLaunchKernelGGL(k_f32_to_bf16, dim3(1024), dim3(256), 0, st, rows_dev, e->sp_g16.p, n);
        CSS_LAUNCH_CHECK();
        rows = e->sp_g16.p;
    }
    return launch_vocab_max(e, rows, cu_dev, B, total_tokens, reinterpret_cast<unsigned*>(zmax_out_dev), st);
}

int css_encoder_forward_sparse(css_encoder* e, const int32_t* ids, const int32_t* cu, int B, int m, int32_t* terms_out,
                               float* weights_out, int32_t* nnz_out, float* dense_out, float* rows_out) {
    CSS_REQUIRE(e && ids && cu && terms_out && weights_out && nnz_out, "css_encoder_forward_sparse: NULL argument");
    CSS_REQUIRE(m >= 1 && m <= kSparseMaxM, "css_encoder_forward_sparse: m=%d outside [1, %d]", m, kSparseMaxM);
    int max_len = 0;
    int rc = check_batch(e, ids, cu, B, &max_len);
    if (rc != CSS_OK) return rc;
    const int T = cu[B];
    const size_t H = e->cfg.hidden, V = e->cfg.vocab;
    std::lock_guard<std::mutex> lk(e->mu);
    if ((rc = check_sparse_state(e, "css_encoder_forward_sparse")) != CSS_OK) return rc;
    DeviceGuard g(e->device);
    const size_t bm = (size_t)B * m;
    if ((rc = ensure_acts(e, T, B)) != CSS_OK || (rc = e->sp_z.grow((size_t)B * V)) != CSS_OK ||
        (rc = e->sp_terms.grow(bm)) != CSS_OK || (rc = e->sp_w.grow(bm)) != CSS_OK || (rc = e->sp_nnz.grow(B)) != CSS_OK)
        return rc;
    hipStream_t st = e->stream;
    CSS_HIP_TRY(hipMemcpyAsync(e->ids_dev, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(e->cu_dev, cu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
    // eager launches (the tiny-batch graphs replay css_encoder_forward only)
    if ((rc = forward_sparse_any(e, e->ids_dev, e->cu_dev, B, T, max_len, m, e->sp_terms.p, e->sp_w.p, e->sp_nnz.p, e->sp_z.p,
                                 e->pre32, st)) != CSS_OK)
        return rc;
    CSS_HIP_TRY(hipMemcpyAsync(terms_out, e->sp_terms.p, bm * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipMemcpyAsync(weights_out, e->sp_w.p, bm * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipMemcpyAsync(nnz_out, e->sp_nnz.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    if (dense_out) CSS_HIP_TRY(hipMemcpyAsync(dense_out, e->sp_z.p, (size_t)B * V * 4, hipMemcpyDeviceToHost, st));
    if (rows_out) CSS_HIP_TRY(hipMemcpyAsync(rows_out, e->pre32, (size_t)T * H * 4, hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

int css_encoder_forward_sparse_dev(css_encoder* e, const int32_t* ids_dev, const int32_t* cu_dev, int B, int total_tokens,
                                   int max_len, int m, int32_t* terms_out_dev, float* weights_out_dev, int32_t* nnz_out_dev,
                                   float* dense_out_dev, float* rows_out_dev, void* stream) {
    CSS_REQUIRE(e && ids_dev && cu_dev && terms_out_dev && weights_out_dev && nnz_out_dev,
                "css_encoder_forward_sparse_dev: NULL argument");
    CSS_REQUIRE(m >= 1 && m <= kSparseMaxM, "css_encoder_forward_sparse_dev: m=%d outside [1, %d]", m, kSparseMaxM);
    CSS_REQUIRE(B >= 1 && total_tokens >= B, "css_encoder_forward_sparse_dev: bad batch (B=%d, tokens=%d)", B, total_tokens);
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = check_sparse_state(e, "css_encoder_forward_sparse_dev");
    if (rc != CSS_OK) return rc;
    DeviceGuard g(e->device);
    rc = ensure_acts(e, total_tokens, B);
    // (dense_out NULL: the maxima stay in the encoder's own buffer; growing it frees the old one, so work that an
    // earlier call enqueued on another stream must have finished, as for the activations)
    if (rc == CSS_OK && !dense_out_dev) rc = e->sp_z.grow((size_t)B * e->cfg.vocab);
    if (rc != CSS_OK) return rc;
    unsigned* z = dense_out_dev ? reinterpret_cast<unsigned*>(dense_out_dev) : e->sp_z.p;
    return forward_sparse_any(e, ids_dev, cu_dev, B, total_tokens, max_len, m, terms_out_dev, weights_out_dev, nnz_out_dev, z,
                              rows_out_dev ? rows_out_dev : e->pre32, (hipStream_t)stream);
}

}  // extern "C"
