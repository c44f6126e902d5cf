// css_index.hip -- exact flat index (IndexFlatIP / IndexFlatL2 semantics) for gfx950.
//
// Replaces, behind include/css_hip.h, the faiss calls of the reference's
// HybridStorage: index creation (src/storage.py:252-258), add with the fused
// row normalisation (src/storage.py:343-359) and the brute-force search
// (src/storage.py:424-436).
//
// HBM layout: xb[cap][dpad] fp32 row-major, dpad = dim rounded up to 64 floats
// (768 -> 768, i.e. 3072 B rows), zero padded, xnorm2[cap] (squared norms) and,
// for inner-product indexes while it fits, a bf16 shadow copy xh[cap][dpad] of
// the rows (coarse scans read it; see css_knn_coarse.h).  Capacity grows
// geometrically or is reserved up front (css_index_reserve) so a 10M..80M row
// shard is allocated once.
//
// Kernels (DESIGN.md has the rooflines):
//   k_ingest_rows      one wave per row: optional synthetic generation, fused
//                      x/(||x||+1e-8), zero pad, squared norm, bf16 shadow.  HBM bound
//   k_compact_rows     css_index_remove_rows: survivors re-ingested at their new slots, window after
//                      window (k_keep_prefix, k_compact_gather, k_rows_maxima).  HBM bound
//   k_scan_coarse,     default search path: coarse bf16 scores (MFMA scan for
//   k_sweep_coarse,    batches, HBM-bound sweep for 1..4 queries) inside a rigorous
//   k_coarse_select    error band, then exact fp32 rescoring of the band (css_knn_coarse.h)
//   k_scan_small       exact fp32 sweep for 1..16 queries (L2 metric, no shadow rows,
//                      flagged queries): 16 lanes per row, VALU FMAs, DPP row reduction,
//                      block-shared sorted top-k lists in LDS, grid-wide threshold.   HBM bound
//   k_scan_mfma_split  exact batched scan on split bf16 operands (3 MFMAs per product);
//   k_scan_mfma        the same on fp32-input MFMA (CSS_SEARCH_EXACT_FP32, verification)
//   k_merge_final      per query: merge the per-block lists into the final top-k.
//   k_range_small      css_index_range_search: the exact fp32 sweep with a radius test and a variable-length
//                      hit list instead of top-k lists (css_knn_range.h).   HBM bound
//   k_facet_small      css_index_facets: the same sweep with a per-(query, bucket) table of hit counts and best-row
//                      keys instead of the hit list, in LDS per block or in global memory, integer atomics only
//                      (css_knn_facets.h).   HBM bound
//   k_gather_queries,  css_index_search_rows: stored rows copied into a query buffer in front of the ordinary
//   k_drop_self        search for k + 1, and the anchor compacted out of its results behind it (a wave per query)
//   k_collapse_groups, css_index_search_grouped: a pass's results collapsed to the first row of every group label, and
//   k_mask_drop_groups the groups already found dropped from the exclusion bitmap of the next pass (css_knn_group.h)
//   k_scan_prior,      css_index_search_prior: the exact fp32 sweep ranked by score + weight * prior[row], and the raw
//   k_prior_scores     scores of the k returned rows re-formed behind the merge (css_knn_prior.h).   HBM bound
//   k_scan_examples,   css_index_search_examples: the exact fp32 sweep ranked by best positive - gamma * best negative
//   k_example_scores   score over up to 16 example vectors, ONE list; the best positive scores of the k returned rows
//                      re-formed behind the merge (css_knn_examples.h).   HBM bound
//   k_kmeans_assign,   css_index_kmeans_step: one Lloyd step -- rows x centroids on the fp32-input MFMA, member lists,
//   k_kmeans_sum       fixed-point int64 sums (css_kmeans.h)
//   k_gram_fx,         css_index_gram: the fixed-point Gram matrix of the rows on the fp64 matrix core;
//   k_transform_rows   css_index_transform: y = A x + b over stored rows, the K loop of k_kmeans_assign (css_pca.h)
//   k_lex_scores       css_index_search_hybrid: the BM25 column of one query over the per-row term lists, handed to
//                      k_scan_prior in the place of the priors (css_lexical.h).   HBM bound
//   k_sparse_scores,   css_index_search_sparse / _hybrid_sparse: the dot column of one sparse query over the per-row
//   k_sparse_topk      sparse vectors; ranked alone by slices of the column and the part merge, or handed to
//                      k_scan_prior like the BM25 column (css_sparse.h).   HBM bound up to 32 terms
//   k_tok_scores       css_index_search_maxsim / css_index_maxsim_rows: the MaxSim column of one query matrix over the
//                      per-row token matrices, bf16 MFMA with the query in registers, a persistent grid; raw matrices
//                      (NB = 0) or COMPRESSED ones (NB = 1, 2, 4), whose B fragment is decoded in registers from codes,
//                      packed buckets and a gathered centroid row; ranked by k_sparse_topk_cols and the part merge.
//                      css_tokens.h, which also holds the ONE copy of the turn's head and tail, the query fragments,
//                      the staged tile and the tile step that k_tok_scores_b and k_tok_ci share.   HBM bound
//   k_tok_encode,      the token codec (css_index_set_token_codec: centroid id + residual buckets per token): the
//   k_tok_decode,      encoder (argmax over centroids on the bf16 MFMA, buckets, packing), the decoder of
//   k_tok_move_units   css_index_set_tokens / _get_tokens and the mover of css_index_remove_rows (css_token_codec.h)
//   k_tok_ctable,      css_index_maxsim_candidates / css_index_search_maxsim_pruned: the query's dots with the codec's
//   k_tok_ci,          centroids, the MaxSim of every row's CENTROIDS from its 2-byte codes and that table, and an exact
//   k_sel_*            multi-block radix select of the best ncand rows in row order (css_token_prune.h); the exact pass
//                      over the candidates is k_tok_scores through its row list
//   k_tok_scores_b     css_index_search_maxsim_batch: the MaxSim columns of a GROUP of 8 query matrices in one pass, raw
//                      or compressed store: a block of 8 waves, one query per wave in registers, every 16-token tile
//                      loaded (and decoded) once per block into an LDS ring in fragment order; ranked by
//                      k_sparse_topk_cols and one part merge per group (css_tokens_batch.h)
//   k_tok_scores_l,    css_index_maxsim_rows_batch / css_index_search_rerank_maxsim: the MaxSim of many query matrices,
//   k_rr_lists,        each over a row list of its own, in one launch (the query belongs to the turn; a wave reloads its
//   k_rr_out           fragments when its turn's query changes); the pool lists of a dense search as row lists, and the
//                      answer from the ranked positions (css_tokens_lists.h)
//   k_sig_count        css_index_subset_terms / _significant_terms: +1 per list entry of the selected rows into a
//                      uint32 table [2^24], repeats merged in a per-block LDS table first; k_sig_score and the radix
//                      select rank the terms (css_sigterms.h)
//   k_mmr_select       css_index_search_diverse: k of a pool of the best rows picked greedily by maximal marginal
//                      relevance, similarities from the stored fp32 rows (css_knn_diverse.h)
//
// Host plumbing, one place per rule: the row storage and every workspace are DevBufs (css_devbuf.h: owning, freed with
// the index, one of three growth policies); a search reads the rows through a Rows value taken under the shared lock
// (rows_of; a row range is Rows::range) and nothing under the shared lock writes a row field of css_index; WsTurn is a
// search's turn at the shared workspaces (wait for the previous stream's event,
// record at the end); CallScope is the lock and device frame of every search entry point and HostCall the whole frame
// of the host ones (allow-bitmap and input up, result rows reserved, results back; pinned staging for small calls);
// prep_queries is the query preparation of every search; sweep_grid is the grid of the exact sweeps, sweep_variant and
// sweep_slots the fan-out of their launchers over TT / METRIC and the 1 / 2 / 8 / 16 query slots, launch_merge_final the
// plain merge behind them; css_knn_plan.h states the rules of the candidate cascade (kind, growth, schedule, error bound,
// tickets) and launch_scan_coarse applies them as named steps over one CascadeCall; RowColumn is a 4-byte-per-row
// column (labels, priors, the attribute slots) and css_index::columns() the list every row operation walks.  The sweep
// body of k_scan_small, k_range_small, k_scan_prior, k_scan_examples and k_facet_small is deliberately NOT shared
// (css_knn_range.h says why).
#include "css_common.h"
#include "css_devbuf.h"
#include "css_knn_kernels.h"
#include "css_knn_plan.h"
#include "../../include/css_synth.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <string>
#include <cfloat>
#include <cmath>
#include <map>
#include <mutex>
#include <memory>
#include <new>
#include <optional>
#include <shared_mutex>
#include <type_traits>
#include <vector>

using namespace css;

// A 4-byte value per row that follows the rows (the group labels, the priors, an attribute): [cap] words, empty until
// first set (column_for_write), every row that was never set at the default -- `fill` in every byte.  Its life is
// stated once:
// column_alloc (first set, capacity growth, compaction), compact_column, column_check / column_for_write / column_get
// (the set and get entry points), and one loop over css_index::columns() each in reallocate_rows, ingest,
// css_index_reset and css_index_remove_rows.
struct RowColumn {
    const int fill;            // 0xFF: -1 as int32, 0x00: 0.0f
    const char* const what;    // in error strings
    DevBuf<int32_t> words;
    template <typename T>
    T* as() const {
        static_assert(sizeof(T) == sizeof(int32_t), "a column holds 4-byte values");
        return reinterpret_cast<T*>(words.p);
    }
};
// An attribute slot (css_index_set_attr): a column with the default -1 / NaN, typed by its first set
struct AttrColumn : RowColumn {
    int type = -1;   // CSS_ATTR_I32 / CSS_ATTR_F32; -1: never set (no memory)
    AttrColumn() : RowColumn{0xFF, "hipMalloc(attribute column)"} {}
};

struct css_index {
    int dim = 0, dpad = 0, metric = 0, device = 0;
    int64_t ntotal = 0, cap = 0, id_base = 0;   // cap: rows the storage below holds (the DevBuf caps are in elements)
    // a mirror of ntotal that css_index_ntotal reads without a lock (it must not wait behind a long add): set_ntotal
    // is the one place that writes the two
    std::atomic<int64_t> ntotal_pub{0};
    // row storage: written and reallocated under the exclusive lock on mu only; a search reads it through a Rows value
    DevBuf<float> xb;              // [cap][dpad]
    DevBuf<float> xnorm2;          // [cap + 256]
    DevBuf<unsigned short> xh;     // bf16 shadow rows [cap + 256][dpad] for the coarse scan (empty: not kept)
    int shadow = -1;               // -1 undecided, 0 off, 1 on (CSS_KNN_SHADOW, HBM headroom)
    int shadow_policy = -1;        // css_index_set_shadow: -1 automatic, 0 never, 1 always
    int search_mode = CSS_SEARCH_AUTO;
    DevBuf<uint32_t> mask_ws;      // device copy of a host bitmap (upload_allow_bits)
    DevBuf<uint32_t> excl_ws;      // k > 128: allow-bitmap minus the rows earlier passes returned
    DevBuf<int> maxn2;             // device, 3 words: bits of max ||row||^2, max ||row - bf16(row)||^2, max ||row - int8(row)||^2 (cz_eps)
    // int8 shadow rows (kept next to the bf16 ones when there is room): signed byte = round(x / s), s = max|x| / 127 per
    // row; read by the 1..4-query sweep and by the int8 MFMA scan of batches
    DevBuf<unsigned char> x8;      // [cap + 256][dpad]
    DevBuf<float> x8s;             // [cap + 256]
    // the per-row columns, part of the row storage: group labels (css_index_set_groups), -1 = a group of its own, and
    // fp32 priors (css_index_set_priors), 0 = no boost
    RowColumn labels{0xFF, "hipMalloc(group labels)"};
    RowColumn priors{0x00, "hipMalloc(priors)"};
    // ... and the attribute slots that css_index_where and css_index_facets_attr read; a slot that was never set is a
    // null pointer to every loop over columns()
    AttrColumn attrs[CSS_MAX_ATTRS];
    static constexpr int kColumns = 2 + CSS_MAX_ATTRS;
    std::array<RowColumn*, kColumns> columns() {
        std::array<RowColumn*, kColumns> all{&labels, &priors};
        for (int s = 0; s < CSS_MAX_ATTRS; ++s) all[2 + s] = &attrs[s];
        return all;
    }
    // per-row term lists (css_index_set_terms, css_lexical.h): the leading lex_rows rows own entries
    // [lex_off[r], lex_off[r + 1]) of lex_ent and a length lex_dl[r]; lex_df [CSS_TERM_SPACE] and lex_total [1] are the
    // statistics.  All empty until terms are first set (lex_df.p tells).  The buffers are sized by the lists, not by
    // cap, so capacity growth and appended rows leave them alone; reset and css_index_remove_rows follow the rows.
    // lex_off_h mirrors the offsets on the host (the new offsets of a compaction are a host prefix sum)
    DevBuf<uint32_t> lex_ent, lex_dl, lex_df;
    DevBuf<int64_t> lex_off;
    DevBuf<unsigned long long> lex_total;
    std::vector<int64_t> lex_off_h;
    int64_t lex_rows = 0;
    // per-row sparse vectors (css_index_set_sparse, css_sparse.h), independent of the term lists: the leading sp_rows
    // rows own entries [sp_off[r], sp_off[r + 1]) of sp_ent, 8 bytes each (term | weight bits << 32).  No statistics.
    // All empty until vectors are first set (sp_off_h.empty() tells); sp_off_h mirrors the offsets on the host
    DevBuf<unsigned long long> sp_ent;
    DevBuf<int64_t> sp_off;
    std::vector<int64_t> sp_off_h;
    int64_t sp_rows = 0;
    // per-row token matrices (css_index_set_tokens, css_tokens.h), a third list kind: the leading tk_rows rows own
    // tokens [tk_off[r], tk_off[r + 1]) of tk_tok, tk_dim bf16 each.  All empty until matrices are first set
    // (tk_off_h.empty() tells); tk_off_h mirrors the offsets on the host.  tk_blocks: css_index_set_token_blocks
    DevBuf<unsigned short> tk_tok;
    DevBuf<int64_t> tk_off;
    std::vector<int64_t> tk_off_h;
    int64_t tk_rows = 0;
    int tk_dim = 0;
    int tk_blocks = 0;
    // the token codec (css_index_set_token_codec, css_token_codec.h): tk_bits != 0 says that the index has one.  Then
    // the matrices are stored COMPRESSED: tk_code [ntok] and tk_res [ntok, tk_dim * tk_bits / 8] in place of tk_tok,
    // under the same offsets.  tk_cent bf16 [tk_ncent, tk_cdim]; tk_cw fp32 [32] = cutoffs [16] | weights [16], zeros
    // behind the used entries; the *_h vectors mirror them on the host.  The codec outlives the matrices
    DevBuf<unsigned short> tk_cent, tk_code;
    DevBuf<float> tk_cw;
    DevBuf<unsigned char> tk_res;
    std::vector<uint16_t> tk_cent_h;
    std::vector<float> tk_cw_h;
    int tk_bits = 0, tk_ncent = 0, tk_cdim = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    // reusable workspaces (DevBuf: grown on demand, freed with the index; guarded by ws_mu)
    DevBuf<float> q_raw;                // floats
    DevBuf<float> qpad;                 // floats
    DevBuf<float> qnorm2;               // floats
    DevBuf<float> qerr2;                // per query: ||q - bf16(q)||^2 (cz_eps)
    DevBuf<float> qerr2_i8;             // per query: ||q - int8(q)||^2 (int8 MFMA scan)
    DevBuf<float> qscale;               // per query: scale of its int8 row
    // int8 policy feedback: the flagged count of the last search that read the int8 rows travels to pinned host memory
    // behind the search (no synchronisation); the next search of that kind looks at it when it has landed
    struct I8Feedback {
        int* h_nflag = nullptr;
        hipEvent_t ev = nullptr;
        bool pending = false;
        int nq = 0;        // queries of the search the pending count belongs to
        int backoff = 0;   // searches left on the bf16 rows after an int8 search that flagged too many queries
    };
    I8Feedback fb_batch, fb_sweep;
    DevBuf<unsigned short> qsplit;      // bf16 (h,l) pairs
    DevBuf<int> gthr;                   // ints
    DevBuf<float> part_s;  DevBuf<uint32_t> part_i;   // entries
    DevBuf<char> out_i;                 // bytes, 12 per entry; a call's rows: [nq * k ids | nq * k scores] (reserve_out)
    // pinned staging of the host API for the reference's call shape (one query, k' = 100: 3 KB in, 1.2 KB out): pageable
    // copies of that size cost a staging pass and a wait each
    char* h_stage = nullptr;
    static constexpr size_t kHostStage = 64 * 1024;   // bytes, each way
    static bool fits_host_stage(size_t bytes) { return bytes <= kHostStage; }
    DevBuf<float> stage;                // floats
    // css_index_remove_rows: keep bits and their popcount prefix of ONE window of rows (at most 2 MiB each)
    DevBuf<uint32_t> compact_bits, compact_pre;   // words
    // coarse + rescore path (css_knn_coarse.h)
    DevBuf<unsigned short> qh;          // bf16 queries
    DevBuf<float> cthr;
    DevBuf<int> cand_n;
    DevBuf<int> cflags;                 // [nq_pad] flags | [nq_pad] flagged list | [1] count | [1] fix-up blocks done
    DevBuf<float> cand_s;
    DevBuf<uint32_t> cand_i;
    DevBuf<int> cpace;                  // sibling pacing counters [stage][group]
    DevBuf<int> fs_state;               // k_sweep_cascade: ticket / stage counters / threshold key words
    std::map<const void*, int> fs_occ;  // ... blocks of a k_sweep_cascade instantiation that one CU holds (launch_sweep_cascade_t)
    // device-side exact fix-up of flagged queries (k_scan_small<FIX>): one global list + lock per query
    DevBuf<float> fix_s;  DevBuf<uint32_t> fix_i;     // entries [nq_pad][k]
    DevBuf<int> fix_lock;
    // second coarse pass over flagged queries (launch_scan_coarse): up to kF2Max slots with CZ_CAP2 candidates each
    DevBuf<unsigned short> qh2;         // bf16 rows of the flagged queries
    DevBuf<float> thr2;
    DevBuf<int> rs_work;                // [count | (query, part) items] of the band rescoring
    DevBuf<int> cand_n2;
    DevBuf<float> cand_s2;
    DevBuf<uint32_t> cand_i2;
    DevBuf<int> flagB;                  // [nq_pad] list | [1] count | [1] fix-up blocks done: queries left to the exact sweep
    // shadow-less indexes: bf16 rows of one row range at a time + the per-range top-k lists (search_noshadow_ranges)
    DevBuf<unsigned short> xh_tmp;
    DevBuf<float> x8s_tmp;              // row scales when the scratch rows are int8
    int64_t range_rows = 0;   // css_index_set_range_rows: rows per range (0: from the free HBM, at most 2^24)
    DevBuf<float> rng_d;  DevBuf<int64_t> rng_i;
    const int* last_nswept = nullptr;                    // device counter behind css_index_last_swept
    // css_index_range_search (css_knn_range.h): hit counters of the 16 query slots of a sweep and the hit pool,
    // range_cap() entries (score + row) per slot; grown to the counted size when a sweep overflowed it
    DevBuf<unsigned int> range_cnt;
    DevBuf<float> range_s;  DevBuf<uint32_t> range_i;
    static constexpr int kRangeSlots = 16;   // query slots of one sweep (counters, pool segments)
    size_t range_cap() const { return range_s.cap / kRangeSlots; }
    // css_index_facets (css_knn_facets.h): the table of ONE sweep, at most 2^20 entries -- [E uint64 keys | 16 totals |
    // 16 unbucketed | E uint32 counts] in 8-byte words, zeroed before and copied back after every sweep -- and the
    // device copy of a per-call bucket column [ntotal] (a workspace: uploaded on every call, never index state)
    DevBuf<unsigned long long> facet_tab;
    DevBuf<int32_t> facet_col;
    int64_t facet_lds_entries = -1;     // css_index_set_facet_lds_entries: -1 = the library's rule (facet_lds_fits)
    int64_t last_facet_sweeps = 0, last_facet_lds_sweeps = 0;   // of the last css_index_facets (css_index_last_facet_sweeps)
    // css_index_where (css_where.h): the call's table words, and [2 words of count | ceil(ntotal / 32) result words]
    DevBuf<uint32_t> where_tab, where_out;
    // css_index_search_rows: the gathered query rows [nq, dim] (not q_raw: the host search copies into that before it
    // has waited for ws_ev), one invalid-id flag per query, the search's own [nq, k + 1] results in front of
    // k_drop_self, and the device copy of a host id list
    DevBuf<float> rowq;                 // floats
    DevBuf<int> rowq_flag;
    DevBuf<float> rowq_d;               // entries
    DevBuf<int64_t> rowq_i;
    DevBuf<int64_t> rowq_ids;
    // css_index_search_grouped: the [nq, kk] results of a pass, the groups found so far ([nq, k] labels next to the
    // call's output rows) and per query [group count | exhausted flag]
    DevBuf<float> grp_d;                // entries
    DevBuf<int64_t> grp_i;
    DevBuf<int32_t> grp_l;
    DevBuf<int> grp_state;              // [nq] counts | [nq] flags
    int64_t last_group_passes = 0;      // search passes of the last grouped call (css_index_last_group_passes)
    // css_index_search_diverse: the [nq, fetch] pool lists of the search in front of k_mmr_select
    DevBuf<float> div_d;                // entries
    DevBuf<int64_t> div_i;
    // css_index_search_prior: the raw scores [nq, k] of the returned rows, the trailing 4-byte column of the call's
    // results (float bits in HostCall's int32 column)
    DevBuf<int32_t> pri_s;              // entries
    // css_index_search_examples: S = the best positive score [k] of the returned rows, the same 4-byte column
    DevBuf<int32_t> ex_s;               // entries
    // css_index_search_hybrid: the lexical column [ntotal] of the call's query, and [S | L] of the k returned rows, the
    // trailing 4-byte columns of the call's results; css_index_term_stats: the asked terms and [m df | total_len]
    DevBuf<float> lex_col;
    DevBuf<int32_t> hyb_sl;             // 2 k entries
    DevBuf<uint32_t> lex_ask;
    DevBuf<long long> lex_stat;
    // css_index_search_sparse: the query's [terms | weights], and the part lists [blocks, k] of k_sparse_topk (the
    // column itself is lex_col, as in the hybrid search)
    DevBuf<float> sp_q;
    DevBuf<float> sp_pd;
    DevBuf<int64_t> sp_pi;
    // css_index_search_maxsim / css_index_maxsim_rows: the query matrix [mq, P] bf16, the row numbers and the column
    // of a row list (a search's column is lex_col, its part lists sp_pd / sp_pi)
    DevBuf<unsigned short> tk_q;
    DevBuf<uint32_t> tk_ids;
    DevBuf<float> tk_col;
    // css_index_search_maxsim_batch: [offsets | matrices] of the batch as uploaded, and the scans of its last call
    DevBuf<uint32_t> tk_bq;
    int last_maxsim_passes = 0;
    // css_index_search_rerank_maxsim: [dense queries | offsets | matrices] as uploaded, the [nq, fetch] pool lists of
    // the search, their row numbers and MaxSim column, and [S | R] of the returned rows, the trailing 4-byte columns
    // of the call's results (the ranked positions are sp_pd / sp_pi)
    DevBuf<uint32_t> rr_in, rr_rows;
    DevBuf<float> rr_d, rr_col;
    DevBuf<int64_t> rr_i;
    DevBuf<int32_t> rr_sr;
    // css_index_maxsim_candidates / css_index_search_maxsim_pruned (css_token_prune.h): the centroid table [C][16 MT] of
    // the call's query (at most 16 MB), the candidate rows and their approximate scores [ncand], and the select's words
    // [4 x 256 bins | threshold key, need, all, count | 2 per block of the compaction].  The approximate column is
    // lex_col, the exact one of the candidates tk_col, the part lists sp_pd / sp_pi
    DevBuf<float> tk_ctab, tk_capx;
    DevBuf<uint32_t> tk_cand, tk_sel;
    // css_index_kmeans_step (css_kmeans.h): the uploaded centroids [nc, dim]; their padded table [ncpad][dpad] with the
    // squared norms [ncpad] behind it; assignment and distance of every row; the member lists [ntotal] with
    // [nc + 1 offsets | nc + 1 block numbers | nc cursors]; and [KM_HDR words | nc counts | nc * dim sums] of int64
    DevBuf<float> km_craw, km_ctab, km_dist;
    DevBuf<int32_t> km_assign;
    DevBuf<uint32_t> km_members, km_off;
    DevBuf<long long> km_out;
    // css_index_gram (css_pca.h): [GR_HDR words | gp column sums | gp * gp matrix] of int64, gp = dpad rounded up to 128.
    // css_index_transform: the uploaded [A | b] ([m, dim] then [m]); the padded table [mpad][dpad] with its squared
    // norms [mpad] (unused) and the padded bias [mpad] behind it; and one batch of results [rows, m]
    DevBuf<long long> gr_out;
    int64_t gram_rows = 0;   // css_index_set_gram_rows: rows per block of k_gram_fx (0: the rule of gram_enqueue)
    DevBuf<float> tr_raw, tr_tab, tr_y;
    // css_index_subset_terms / css_index_significant_terms (css_sigterms.h): the count tables [CSS_TERM_SPACE] of the
    // selection and of a background mask (64 MB each, allocated on first use; workspaces, not index state), the device
    // copy of the background bitmap, the candidate list (score bits, term) of the select -- also the (term, count)
    // pairs of the compaction --, the SigState and the packed results
    DevBuf<uint32_t> sig_fg, sig_bg, sig_mask2, sig_term, sig_cnt;
    DevBuf<unsigned long long> sig_key, sig_st, sig_out;
    int sig_slots = -1;   // css_index_set_sigterm_slots: LDS slots per block of k_sig_count (-1: the library's rule)
    // rows written by css_index_add_dev / _add_synthetic on the CALLER's stream: searches, reallocation and
    // export wait for this event before touching rows, norms or maxn2
    hipEvent_t ingest_ev = nullptr;
    bool ingest_pending = false;
    // every search shares ONE set of workspaces (qpad, gthr, cthr, cand_*, cflags, fix_*, part_*): ws_mu serialises the
    // host-side enqueue only, so the last search's stream is remembered and a search on ANOTHER stream first waits
    // for this event (recorded at the end of each search) before it overwrites them
    hipEvent_t ws_ev = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_pending = false;
    const int* last_nflag = nullptr;   // device counter of the last candidate-path search (css_index_last_flagged)
    std::shared_mutex mu;  // search: shared; add/reset/reserve: exclusive
    std::mutex ws_mu;      // workspaces + own stream are single-user
};

namespace {

// What a search reads of the rows, as a value: taken once per entry point under the shared lock on mu (rows_of),
// handed down to every launcher next to `ix`, never written back.  mask: the device allow-bitmap of the call, one
// bit per row (null: every row allowed).
struct Rows {
    const float* xb;
    const float* xnorm2;
    const unsigned short* xh;
    const unsigned char* x8;
    const float* x8s;
    int64_t n, id_base;
    const uint32_t* mask;
    const int32_t* labels;   // group labels, one per row (null: none were ever set)
    const float* priors;     // per-row priors (null: none were ever set, every prior is 0)
    // rows [row0, row0 + cnt) as rows of their own, with the range's bf16 OR int8 scratch rows as their shadow (the
    // other kind null): search_noshadow_ranges
    Rows range(int64_t row0, int64_t cnt, int dpad, const unsigned short* xh_rows, const unsigned char* x8_rows,
               const float* x8_scales) const {
        return Rows{xb + (size_t)row0 * dpad, xnorm2 + row0, xh_rows, x8_rows, x8_scales, cnt, id_base + row0,
                    mask ? mask + row0 / 32 : nullptr, labels ? labels + row0 : nullptr,
                    priors ? priors + row0 : nullptr};   // (row0 is a multiple of 256)
    }
};
// the one place that reads the row fields of the index for a search; caller holds mu (shared is enough)
Rows rows_of(const css_index* ix, const uint32_t* mask = nullptr) {
    return Rows{ix->xb.p, ix->xnorm2.p, ix->xh.p, ix->x8.p, ix->x8s.p, ix->ntotal, ix->id_base, mask, ix->labels.words.p,
                ix->priors.as<float>()};
}
// caller holds mu exclusively
void set_ntotal(css_index* ix, int64_t n) {
    ix->ntotal = n;
    ix->ntotal_pub.store(n);
}

constexpr int kWaves = 4;  // waves per block in the scan kernels

// ------------------------------------------------------------------ ingest
// One wave per row.  SYNTH: value = css_synth_normal(seed, (first_row+row)*dim + c).
// STORE = false: nothing but the running maxima is written (dst unused; pass norm2 / dsth / err2_out / dst8 as null):
// css_index_remove_rows re-measures the rows it leaves in place with the arithmetic of the ingest.
template <bool SYNTH, bool STORE = true>
__device__ __forceinline__ void ingest_row(int64_t row, int lane, const float* __restrict__ src, float* __restrict__ dst,
                                           float* __restrict__ norm2, int dim, int dpad, int normalize, uint64_t seed,
                                           int64_t first_row, unsigned short* __restrict__ dsth, int* __restrict__ maxn2,
                                           float* __restrict__ err2_out, unsigned char* __restrict__ dst8,
                                           float* __restrict__ dst8s) {
    const float* s = SYNTH ? nullptr : src + row * (int64_t)dim;
    const uint64_t base = (uint64_t)((first_row + row) * (int64_t)dim);
    float ss = 0.f, amax = 0.f;
    for (int c = lane; c < dim; c += 64) {
        float v = SYNTH ? css_synth_normal(seed, base + (uint64_t)c) : s[c];
        ss = fmaf(v, v, ss);
        amax = fmaxf(amax, fabsf(v));
    }
    ss = wave_allsum(ss);
    amax = wave_allmax(amax);
    // reference: x / (||x||_2 + 1e-8)  (src/storage.py:349-350, :426)
    const float nrm = sqrtf(ss) + 1e-8f;
    float* d = STORE ? dst + row * (int64_t)dpad : nullptr;
    // int8 shadow row: byte = rint(v / s8), s8 = max|v| / 127 (of the values as stored, i.e. after normalisation)
    if (normalize) amax = amax / nrm;
    const float s8 = amax > 0.f ? amax / 127.f : 1.f, inv8 = amax > 0.f ? 127.f / amax : 0.f;
    float e8 = 0.f;
    float s2 = 0.f, e2 = 0.f;
    for (int c = lane; c < dpad; c += 64) {
        float v = 0.f;
        if (c < dim) {
            v = SYNTH ? css_synth_normal(seed, base + (uint64_t)c) : s[c];
            if (normalize) v = v / nrm;
        }
        if (STORE) d[c] = v;
        const __bf16 h = (__bf16)v;   // the rounding every bf16 copy of this row uses (shadow rows, k_rows_to_bf16*)
        if (dsth) dsth[row * (int64_t)dpad + c] = __builtin_bit_cast(unsigned short, h);
        s2 = fmaf(v, v, s2);
        const float dv = v - (float)h;   // exact in fp32
        e2 = fmaf(dv, dv, e2);
        {   // (measured whether or not the int8 row is kept: shadow-less indexes quantise the same way per search)
            const float k8 = fminf(fmaxf(rintf(v * inv8), -127.f), 127.f);
            if (dst8) dst8[row * (int64_t)dpad + c] = (unsigned char)((int)k8 & 0xFF);   // signed int8 (what the int8 MFMA takes)
            const float d8 = fmaf(-s8, k8, v);   // v - s8 * k8 with one rounding
            e8 = fmaf(d8, d8, e8);
        }
    }
    s2 = wave_allsum(s2);
    e2 = wave_allsum(e2);
    e8 = wave_allsum(e8);
    if (lane == 0) {
        if (dst8) dst8s[row] = s8;
        if (maxn2 && e8 > __int_as_float(__hip_atomic_load(maxn2 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
            atomicMax(maxn2 + 2, __float_as_int(e8));
    }
    if (lane == 0 && norm2) norm2[row] = s2;
    // ||row - bf16(row)||^2: what the rounding actually cost (cz_eps: the measured error band of the candidate scans)
    if (lane == 0 && err2_out) err2_out[row] = e2;
    if (lane == 0 && maxn2 && e2 > __int_as_float(__hip_atomic_load(maxn2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
        atomicMax(maxn2 + 1, __float_as_int(e2));
    // running max of ||row||^2 (non-negative floats order like their bit patterns); rows are ~unit
    // norm in the product, so after the first few rows almost no atomic is issued
    if (lane == 0 && maxn2 && s2 > __int_as_float(__hip_atomic_load(maxn2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
        atomicMax(maxn2, __float_as_int(s2));
}
template <bool SYNTH>
__global__ __launch_bounds__(256) void k_ingest_rows(const float* __restrict__ src, float* __restrict__ dst,
                                                     float* __restrict__ norm2, int64_t n, int dim, int dpad,
                                                     int normalize, uint64_t seed, int64_t first_row,
                                                     unsigned short* __restrict__ dsth, int* __restrict__ maxn2,
                                                     float* __restrict__ err2_out, unsigned char* __restrict__ dst8,
                                                     float* __restrict__ dst8s) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    ingest_row<SYNTH>(row, threadIdx.x & 63, src, dst, norm2, dim, dpad, normalize, seed, first_row, dsth, maxn2, err2_out, dst8,
                      dst8s);
}

// ------------------------------------------------------------------ remove rows (css_index_remove_rows)
// In-place stream compaction of the rows behind the first removed one, window after window (the host plans the
// windows: css_index_remove_rows; DESIGN.md "remove_ids" has the hazard argument).  `bits` / `pre` cover ONE window:
// bit (r & 31) of bits[r >> 5] set = row r of the window survives, pre[w] = survivors of the window in words < w.
constexpr int64_t kCompactWindowRows = 1ll << 24;   // rows per launch (one wave per row, as ingest())
constexpr int64_t kCompactWords = kCompactWindowRows / 32;

// Exclusive popcount prefix over the keep words of one window; ONE block of 1024 threads (<= 2 MB of words).
__global__ __launch_bounds__(1024) void k_keep_prefix(const uint32_t* __restrict__ bits, uint32_t* __restrict__ pre, int words) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (words + 1023) / 1024;
    const int w0 = min(t * per, words), w1 = min(w0 + per, words);
    uint32_t s = 0;
    for (int w = w0; w < w1; ++w) s += (uint32_t)__popc(bits[w]);
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // Hillis-Steele inclusive scan
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int w = w0; w < w1; ++w) {
        pre[w] = run;
        run += (uint32_t)__popc(bits[w]);
    }
}

// window-local number of the surviving row r among the survivors, or -1 (wave-uniform)
__device__ __forceinline__ int64_t compact_slot(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre, int64_t r) {
    const uint32_t w = bits[r >> 5];
    const int b = (int)(r & 31);
    if (!((w >> b) & 1u)) return -1;
    return (int64_t)pre[r >> 5] + __popc(w & ((1u << b) - 1u));
}

// One wave per row of the window.  Survivor r (every row when bits is null): fp32 row read at src + r * dpad, and
// the row re-ingested (normalize = 0) at slot `compact_slot` of the destination arrays: ingest_row writes the fp32 row,
// its norm and the shadow rows the index keeps, and raises the three maxima -- the bits of an ingest of that row.
// The caller guarantees that no destination slot of the launch is a source row of the launch.
__global__ __launch_bounds__(256) void k_compact_rows(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre,
                                                      int64_t n, const float* src, float* dst, float* norm2, int dim, int dpad,
                                                      unsigned short* dsth, int* __restrict__ maxn2, unsigned char* dst8,
                                                      float* dst8s) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t o = bits ? compact_slot(bits, pre, r) : r;
    if (o < 0) return;
    ingest_row<false>(0, threadIdx.x & 63, src + r * (int64_t)dpad, dst + o * (int64_t)dpad, norm2 + o, dim, dpad, 0, 0ull, 0ll,
                      dsth ? dsth + o * (int64_t)dpad : nullptr, maxn2, (float*)nullptr, dst8 ? dst8 + o * (int64_t)dpad : nullptr,
                      dst8 ? dst8s + o : nullptr);
}

// Bounce, first half: the fp32 rows of the window's survivors, packed into the scratch rows (16 bytes per lane, whole
// 128-byte lines; the scratch is read again at once by k_compact_rows, so plain stores).
__global__ __launch_bounds__(256) void k_compact_gather(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre,
                                                        int64_t n, const float* __restrict__ src, float* __restrict__ scratch,
                                                        int dpad) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t o = compact_slot(bits, pre, r);
    if (o < 0) return;
    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    const nt_f4* s = reinterpret_cast<const nt_f4*>(src + r * (int64_t)dpad);
    nt_f4* d = reinterpret_cast<nt_f4*>(scratch + o * (int64_t)dpad);
    for (int c = threadIdx.x & 63; c < dpad / 4; c += 64) d[c] = __builtin_nontemporal_load(s + c);
}

// The rows that stay where they are (below the first removed row): the three maxima only, nothing written to the rows.
__global__ __launch_bounds__(256) void k_rows_maxima(const float* __restrict__ rows, int64_t n, int dim, int dpad,
                                                     int* __restrict__ maxn2) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    ingest_row<false, false>(0, threadIdx.x & 63, rows + r * (int64_t)dpad, (float*)nullptr, (float*)nullptr, dim, dpad, 0, 0ull,
                             0ll, (unsigned short*)nullptr, maxn2, (float*)nullptr, (unsigned char*)nullptr, (float*)nullptr);
}

// ------------------------------------------------------------------ scan (small nq)
// Block = 4 waves.  A wave instruction covers 4 rows: lane = 16*r + sub reads the
// float4 at column 64*t + 4*sub of row r, so 16 lanes fetch 256 contiguous bytes.
// Scores are "larger is better": IP -> dot, L2 -> -(sum (x-q)^2).
// LDS: qs[NQ][dpad] | ls[NQ][k] | li[NQ][k] | lock[NQ] | qid[NQ] | (FIX) per-wave merge scratch
//
// FIX = true is the device-side exact fix-up of the candidate path (css_knn_coarse.h): the launch follows
// every cascade unconditionally, reads the number of flagged queries from device memory and returns at once
// when it is zero (the usual case) -- no host round trip.  Otherwise the grid walks the flagged queries NQ at
// a time; a block's lists are merged into one global list per query under an agent-scope lock (release /
// acquire fences around plain loads and stores, MI355X_MICROARCH.md "Valid forms"); the lists were reset by
// the kernel that flagged the query; the block that finishes last turns them into D / I rows.
// (rows are read once per sweep: non-temporal, like the shadow-row sweeps -- css_knn_coarse.h, cz_row_load; CSS_SCAN_NT=0 builds for A/B runs)
#ifndef CSS_SCAN_NT
#define CSS_SCAN_NT 1
#endif
__device__ __forceinline__ float4 scan_row_load(const float4* p) {
#if CSS_SCAN_NT
    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
template <int NQ, int TT, int METRIC, bool FIX = false>
__global__ __launch_bounds__(256, 4) void k_scan_small(const float4* __restrict__ xb, const float* __restrict__ qpad,
                                                    int64_t ntotal, int T_rt, int k, int64_t groups_per_block,
                                                    int* __restrict__ gthr, float* __restrict__ part_s,
                                                    uint32_t* __restrict__ part_i, int nq_real_arg,
                                                    const uint32_t* __restrict__ mask,
                                                    const int* __restrict__ flag_list, const int* __restrict__ nflag_p,
                                                    float* fix_s, uint32_t* fix_i, int* fix_lock, int* fix_done,
                                                    int64_t id_base, float* D, int64_t* I) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = TT > 0 ? TT : T_rt;  // float4 steps of 16 lanes: dpad = 64*T
    const int dpad = T * 64;
    float* qs = reinterpret_cast<float*>(smem);
    float* ls = qs + NQ * dpad;
    uint32_t* li = reinterpret_cast<uint32_t*>(ls + NQ * k);
    int* lock = reinterpret_cast<int*>(li + NQ * k);
    int* qid = lock + NQ;                                   // query served by list j
    float* ms = reinterpret_cast<float*>(qid + NQ);         // FIX: [4 waves][k] merge scratch
    uint32_t* mi = reinterpret_cast<uint32_t*>(ms + 4 * k);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rsub = lane >> 4;
    const int nfl = FIX ? __hip_atomic_load(nflag_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1;
    if (FIX && nfl == 0) return;

  for (int c0 = 0; c0 < (FIX ? nfl : 1); c0 += NQ) {
    const int nq_real = FIX ? min(NQ, nfl - c0) : nq_real_arg;
    if (tid < NQ) {
        lock[tid] = 0;
        qid[tid] = FIX ? (tid < nq_real ? flag_list[c0 + tid] : 0) : tid;
    }
    __syncthreads();
    for (int i = tid; i < NQ * dpad; i += 256) {
        const int j = i / dpad;
        qs[i] = j < nq_real ? qpad[(size_t)qid[j] * dpad + (i - j * dpad)] : 0.f;
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

    float gcache[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) gcache[j] = -INFINITY;
    int iter = 0;

    for (int64_t g = g_begin + wave; g < g_end; g += kWaves, ++iter) {
        // refresh the grid-wide thresholds now and then; kept at the top of the
        // iteration so the FMA block below and its consumers stay in one basic block (stale values only prune less)
        if ((iter & 15) == 0) {
#pragma unroll
            for (int j = 0; j < NQ; ++j)
                gcache[j] = key2f(__hip_atomic_load(&gthr[qid[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }

        const int64_t row = g * 4 + rsub;
        const bool in_range = row < ntotal;
        const int64_t rowc = in_range ? row : ntotal - 1;
        // masked search: rows whose bit is clear can never be candidates (filter / tombstone push-down)
        const bool valid = in_range && (mask == nullptr || ((mask[rowc >> 5] >> (rowc & 31)) & 1u));
        const float4* xr = xb + rowc * (int64_t)(T * 16) + sub;

        float acc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] = 0.f;
        // NQ > 1: keep the query fragments in LDS (re-read per row group) instead of
        // letting LICM pin 12*NQ float4 in VGPRs, which would cost all the occupancy.
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
                // fence the scheduler per column step: otherwise all 12*NQ LDS reads are
                // clustered up front and the kernel spills
                if constexpr (NQ > 1) __builtin_amdgcn_sched_barrier(0);
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

        // All scores and pass flags are formed in this basic block (one combined
        // ballot), so the FMA chains above cannot be sunk behind the rare slow path.
        float sc[NQ];
        bool anyp = false;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float s = row16_allsum(acc[j]);
            if constexpr (METRIC == CSS_METRIC_L2) s = -s;
            sc[j] = s;
            const float lthr = ls[j * k + (k - 1)];
            // non-strict: an equal score with a lower row id must still reach the comparator
            anyp |= (s >= lthr) & (s >= gcache[j]) & (j < nq_real);  // '&': no short-circuit branches
        }
        if (__ballot(anyp && valid && sub == 0) == 0ull) continue;

        for (int j = 0; j < nq_real; ++j) {
            float s = sc[0];
#pragma unroll
            for (int u = 1; u < NQ; ++u) s = j == u ? sc[u] : s;
            const float lthr = ls[j * k + (k - 1)];
            const float gj = key2f(__hip_atomic_load(&gthr[qid[j]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
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
                if (changed && kth > gj) atomicMax(&gthr[qid[j]], f2key(kth));
            }
        }
    }
    __syncthreads();
    if constexpr (FIX) {
        // merge this block's lists into the global list of each query (rare path: clarity over speed)
        float* ws = ms + wave * k;
        uint32_t* wi = mi + wave * k;
        for (int j = wave; j < nq_real; j += kWaves) {
            const int q = qid[j];
            float* gs = fix_s + (size_t)q * k;
            uint32_t* gi = fix_i + (size_t)q * k;
            if (li[j * k] == kInvalidRow) continue;  // nothing found in this block's rows (wave uniform)
            // a lower bound of the global k-th best: lists only improve, so a stale value only merges more
            const float gk = key2f(__hip_atomic_load(&gthr[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (ls[j * k] < gk) continue;
            // All blocks finish their rows at about the same time and queue here with the threshold they saw at the
            // start of the queue.  Every merge raises gthr to the global k-th best, so a waiting block keeps looking
            // at it and leaves the queue as soon as its own best row can no longer enter the list: ~k ln(blocks)
            // merges per query instead of one per block (measured on 1 M clustered rows: 12 ms -> under 1 ms per chunk
            // of 8 flagged queries).
            int give_up = 0;
            if (lane == 0) {
                int expect = 0;
                while (!__hip_atomic_compare_exchange_strong(&fix_lock[q], &expect, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT)) {
                    expect = 0;
                    __builtin_amdgcn_s_sleep(8);
                    if (ls[j * k] < key2f(__hip_atomic_load(&gthr[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                        give_up = 1;
                        break;
                    }
                }
            }
            if (__shfl(give_up, 0)) continue;   // (strictly below the k-th best: ties still merge, lowest ids win)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int i = lane; i < k; i += 64) {
                ws[i] = gs[i];
                wi[i] = gi[i];
            }
            bool changed = false;
            for (int p = 0; p < k; ++p) {
                const uint32_t id = li[j * k + p];
                if (id == kInvalidRow) break;
                if (!wave_insert<uint32_t>(ws, wi, k, ls[j * k + p], id, lane)) break;  // sorted: the rest is worse
                changed = true;
            }
            if (changed) {
                for (int i = lane; i < k; i += 64) {
                    gs[i] = ws[i];
                    gi[i] = wi[i];
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const float kth = ws[k - 1];
            if (lane == 0) {
                if (changed && wi[k - 1] != kInvalidRow) atomicMax(&gthr[q], f2key(kth));
                __hip_atomic_store(&fix_lock[q], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();  // the next chunk re-initialises the LDS lists
    } else {
        // part layout: [q][block][k]
        const int G = gridDim.x;
        for (int i = tid; i < nq_real * k; i += 256) {
            const int j = i / k, p = i - j * k;
            const size_t o = ((size_t)j * G + blockIdx.x) * k + p;
            part_s[o] = ls[i];
            part_i[o] = li[i];
        }
    }
  }
    if constexpr (FIX) {
        // The block that finishes last turns the global lists into the D / I rows of the flagged queries (a launch of
        // its own until round 4: 9 us of every search for nothing, flagged queries being rare).  Every merge above
        // ended with an agent-scope release under the list's lock; the counter add follows this block's last one.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(fix_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == (int)gridDim.x - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            lock[0] = last;
        }
        __syncthreads();
        if (lock[0]) {
            for (int f = 0; f < nfl; ++f) {
                const int q = flag_list[f];
                for (int i = tid; i < k; i += 256) {
                    const uint32_t id = __hip_atomic_load(&fix_i[(size_t)q * k + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const float s = __hip_atomic_load(&fix_s[(size_t)q * k + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // IP: dot; L2: -(squared distance)
                    const bool ok = id != kInvalidRow;
                    D[(size_t)q * k + i] = METRIC == CSS_METRIC_IP ? (ok ? s : -FLT_MAX) : (ok ? -s : FLT_MAX);
                    I[(size_t)q * k + i] = ok ? id_base + (int64_t)id : (int64_t)-1;
                }
            }
        }
    }
}

// Empty index: every slot padded (cannot be reached through the reference: src/storage.py:421-422).
__global__ void k_fill_pad(float* __restrict__ D, int64_t* __restrict__ I, int64_t n, float pad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        D[i] = pad;
        I[i] = -1;
    }
}

// ---- css_index_search_rows: stored rows as queries.  Two bandwidth-trivial launches around the ordinary search.
// One wave per anchor: the fp32 row of global id ids[j] -> raw query row j ([nq, dim], what css_index_search_dev
// takes), 16 bytes per lane where the rows allow it.  An id outside [id_base, id_base + ntotal) reads nothing: its
// query is a zero row and flag[j] = 1 (k_drop_self pads that result row).
__global__ __launch_bounds__(256) void k_gather_queries(const float* __restrict__ xb, const int64_t* __restrict__ ids,
                                                        float* __restrict__ q, int* __restrict__ flag, int64_t nq,
                                                        int64_t ntotal, int64_t id_base, int dim, int dpad) {
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= nq) return;
    const uint64_t r = (uint64_t)ids[j] - (uint64_t)id_base;   // (unsigned: an id below id_base wraps beyond ntotal)
    const bool ok = r < (uint64_t)ntotal;
    if (lane == 0) flag[j] = ok ? 0 : 1;
    const float* src = xb + (ok ? (size_t)r * dpad : 0);
    float* dst = q + (size_t)j * dim;
    if ((dim & 3) == 0) {   // (rows of q then start on 16-byte boundaries like those of xb)
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = lane; c < dim / 4; c += 64)
            reinterpret_cast<float4*>(dst)[c] = ok ? reinterpret_cast<const float4*>(src)[c] : zero;
    } else {
        for (int c = lane; c < dim; c += 64) dst[c] = ok ? src[c] : 0.f;
    }
}

// One wave per query: stable compaction of its kk = k + (exclude ? 1 : 0) sorted results to k.  exclude: the entry
// whose id is the anchor's goes if it is there, otherwise the last one does (ids are unique inside a row, so at most
// one entry goes and k always remain; the pads of a short row travel along).  A flagged query is padded entirely.
__global__ __launch_bounds__(256) void k_drop_self(const float* __restrict__ Ds, const int64_t* __restrict__ Is,
                                                   const int64_t* __restrict__ ids, const int* __restrict__ flag,
                                                   int64_t nq, int kk, int k, int exclude, float pad,
                                                   float* __restrict__ D, int64_t* __restrict__ I) {
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= nq) return;
    float* Dj = D + (size_t)j * k;
    int64_t* Ij = I + (size_t)j * k;
    int kept = 0;
    if (!flag[j]) {
        const int64_t anchor = ids[j];
        for (int c0 = 0; c0 < kk; c0 += 64) {
            const int c = c0 + lane;
            const bool in = c < kk;
            const int64_t id = in ? Is[(size_t)j * kk + c] : -1;
            const float s = in ? Ds[(size_t)j * kk + c] : pad;
            const bool keep = in && !(exclude && id == anchor);
            const unsigned long long b = __ballot(keep);
            const int pos = kept + __popcll(b & ((1ull << lane) - 1ull));
            if (keep && pos < k) {
                Dj[pos] = s;
                Ij[pos] = id;
            }
            kept += __popcll(b);
        }
    }
    for (int c = kept + lane; c < k; c += 64) {
        Dj[c] = pad;
        Ij[c] = -1;
    }
}


// ------------------------------------------------------------------ scan (query batches, MFMA)
// C[128 rows x 128 queries] = X[128 x 768] * Q^T on v_mfma_f32_32x32x2_f32 (exact
// fp32 fmaf chains, 157 TFLOP/s dense peak).  Block = 4 waves; wave w owns query
// columns [32w, 32w+32) x all 128 rows = 4 accumulator tiles (64 AGPR/VGPR).
// Per K-step (BK = 32 floats): X tile and Q tile are staged global -> registers
// -> LDS (double buffered, one barrier per step, loads for step t+1 in flight
// during the MFMAs of step t).  LDS rows are 128 B; the 16-B chunk index is
// XOR-swizzled with (row>>1)&7 so every ds_read_b128 lane group hits 16
// different slots of the 256-B bank row.
// After the last K-step of a row tile the epilogue compares the 64 scores a lane
// holds (one query column per lane) with that query's current k-th best; only
// when something passes is the tile spilled to an LDS scratch and inserted into
// the wave-owned sorted lists.  Thresholds are also exchanged grid-wide (gthr).
constexpr int MF_BM = 128, MF_BN = 128, MF_BK = 32;
#ifndef CSS_MF_LAG
#define CSS_MF_LAG 12
#endif
#ifndef CSS_MF_POLL
#define CSS_MF_POLL 8   // (a power of two)
#endif
constexpr int MF_LAG = CSS_MF_LAG;   // K-steps a block may run ahead of its slowest sibling (k_scan_mfma pacing)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));  // plain clang vector: stays in VGPRs

__device__ __forceinline__ int mf_swz(int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 1) & 7)) << 2); }

template <int METRIC>
__global__ __launch_bounds__(256, 1) void k_scan_mfma(const float* __restrict__ xb, const float* __restrict__ xnorm2,
                                                      const float* __restrict__ qpad, int nq_real, int64_t ntotal,
                                                      int dpad, int k, int nstrips, int nqtiles,
                                                      int64_t tiles_per_strip, int* __restrict__ gthr,
                                                      float* __restrict__ part_s, uint32_t* __restrict__ part_i,
                                                      const uint32_t* __restrict__ mask, int* __restrict__ pace) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* As = reinterpret_cast<float*>(smem);                 // [2][128][32]
    float* Bs = As + 2 * MF_BM * MF_BK;                         // [2][128][32]
    float* scr = Bs + 2 * MF_BN * MF_BK;                        // [4 waves][32][33]
    float* xn2s = scr + 4 * 32 * 33;                            // [128]
    float* ls = xn2s + MF_BM;                                   // [128][k]
    uint32_t* li = reinterpret_cast<uint32_t*>(ls + MF_BN * k);  // [128][k]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware decode: blocks l, l+8, l+16, ... (same XCD under round-robin dispatch)
    // walk the query tiles of ONE strip, so the strip's rows are fetched once per XCD L2.
    const int l = blockIdx.x;
    const int strip = (l / (8 * nqtiles)) * 8 + (l & 7);
    const int qtile = (l >> 3) % nqtiles;
    const int64_t ntiles = (ntotal + MF_BM - 1) / MF_BM;
    const int64_t t_begin = (int64_t)strip * tiles_per_strip;
    const int64_t t_end = min(t_begin + tiles_per_strip, ntiles);
    const int q_base = qtile * MF_BN;

    for (int i = tid; i < MF_BN * k; i += 256) {
        ls[i] = -INFINITY;
        li[i] = kInvalidRow;
    }
    __syncthreads();
    if (t_begin >= t_end) {
        for (int i = tid; i < MF_BN * k; i += 256) {
            const int j = i / k, p = i - j * k;
            if (q_base + j < nq_real) {
                const size_t o = ((size_t)(q_base + j) * nstrips + strip) * k + p;
                part_s[o] = -INFINITY;
                part_i[o] = kInvalidRow;
            }
        }
        return;
    }

    const int KT = dpad / MF_BK;
    const int64_t n_it = (t_end - t_begin) * KT;
    // staging map: thread -> (row = (tid>>3) + 32*i, 16-B chunk = tid&7), i = 0..3
    const int srow = tid >> 3, schunk = tid & 7;
    v4f ra[4], rb[4];

// (macros, not lambdas: by-reference lambda captures left ra/rb in scratch memory)
#define MF_GLOAD(RT, KT)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        int64_t row_ = (RT) * MF_BM + srow + 32 * i;                                                         \
        row_ = row_ < ntotal ? row_ : ntotal - 1;                                                            \
        ra[i] = *reinterpret_cast<const v4f*>(xb + row_ * (int64_t)dpad + (KT) * MF_BK + schunk * 4);     \
        rb[i] = *reinterpret_cast<const v4f*>(qpad + (int64_t)(q_base + srow + 32 * i) * dpad +           \
                                                 (KT) * MF_BK + schunk * 4);                                 \
    }
#define MF_SSTORE(BUF)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        *reinterpret_cast<v4f*>(As + (BUF) * MF_BM * MF_BK + mf_swz(srow + 32 * i, schunk)) = ra[i];      \
        *reinterpret_cast<v4f*>(Bs + (BUF) * MF_BN * MF_BK + mf_swz(srow + 32 * i, schunk)) = rb[i];      \
    }

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    const int jq = wave * 32 + fr;  // this lane's query column inside the tile
    float thr_g = -INFINITY;

    MF_GLOAD(t_begin, 0)
    MF_SSTORE(0)
    __syncthreads();
    int cur = 0;
    int64_t rt = t_begin;  // row tile / K-step of the tile being computed
    int kt = 0;
    for (int64_t it = 0; it < n_it; ++it) {
        // Sibling pacing: the nqtiles blocks of a strip sit on one XCD and read the same rows.  Every CSS_MF_POLL-th
        // K-step a block publishes its step count and looks at its siblings'; it does not run more than MF_LAG steps
        // ahead of the slowest, so a K-step of rows (16 KB) is still in that XCD's L2 when the others ask for it.
        // Unpaced, the siblings drift apart with their insert work and each fetches the strip from HBM again.
        // Measured at 10 M rows x 256 queries (rocprofv3 --pmc FETCH_SIZE, 30.72 GB algorithmic): unpaced 52.0 GB
        // (1.69 x) in 49.0 ms; poll 8 / lag 12: 34.0 GB (1.11 x) in 50.6 ms; poll 4 / lag 8: 33.2 GB, 51.9 ms; poll
        // 16 / lag 16: 43.0 GB, 49.8 ms.  The kernel is bound by the fp32 MFMA pipe, not by HBM, so the saved traffic
        // buys no time here (it frees HBM for whatever else runs on the chip).
        // The look is issued here and used after the MFMAs of the step; the spin is bounded, so a sibling that is
        // not resident only costs a wait.
        int sib_lo = 1 << 30;
        const bool pace_now = pace != nullptr && tid == 0 && (it & (CSS_MF_POLL - 1)) == 0;
        if (pace_now) {
            __hip_atomic_store(pace + (size_t)strip * nqtiles + qtile, (int)it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int j = 0; j < nqtiles; ++j)
                sib_lo = min(sib_lo, __hip_atomic_load(pace + (size_t)strip * nqtiles + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        if (it + 1 < n_it) {
            const int64_t nrt = kt + 1 < KT ? rt : rt + 1;
            const int nkt = kt + 1 < KT ? kt + 1 : 0;
            MF_GLOAD(nrt, nkt)
        }
        const float* A = As + cur * MF_BM * MF_BK;
        const float* B = Bs + cur * MF_BN * MF_BK;
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // 8 k-values per chunk pair: lane half fh takes chunk 2c+fh
            const v4f b = *reinterpret_cast<const v4f*>(B + mf_swz(jq, 2 * c + fh));
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
        if (kt == KT - 1) {
            // ---------------- epilogue of row tile rt ----------------
            const int64_t row0 = rt * MF_BM;
            if constexpr (METRIC == CSS_METRIC_L2) {
                // s = 2 x.q - ||x||^2  (||q||^2 is added in the final merge)
                if (tid < MF_BM) xn2s[tid] = row0 + tid < ntotal ? xnorm2[row0 + tid] : 0.f;
                __syncthreads();
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[m][r] = 2.f * acc[m][r] - xn2s[32 * m + (r & 3) + 8 * (r >> 2) + 4 * fh];
            }
            thr_g = key2f(__hip_atomic_load(&gthr[q_base + jq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            float thr_l = ls[jq * k + (k - 1)];
            const float thr = fmaxf(thr_l, thr_g);
            const bool full_tile = row0 + MF_BM <= ntotal;
            bool anyp = false;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) anyp |= acc[m][r] >= thr;
            anyp &= jq + q_base < nq_real;
            if (__ballot(anyp) != 0ull) {
                float* S = scr + wave * (32 * 33);
                bool changed = false;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) S[((r & 3) + 8 * (r >> 2) + 4 * fh) * 33 + fr] = acc[m][r];
                    for (int rr = 0; rr < 32; ++rr) {
                        const int64_t row = row0 + 32 * m + rr;
                        const float sv = S[rr * 33 + fr];
                        const bool pass = fh == 0 && (full_tile || row < ntotal) && q_base + jq < nq_real &&
                                          (mask == nullptr || ((mask[row >> 5] >> (row & 31)) & 1u)) &&
                                          sv >= thr_l && sv >= thr_g;
                        unsigned long long mk = __ballot(pass);
                        if (mk == 0ull) continue;
                        while (mk) {
                            const int src = __ffsll((long long)mk) - 1;
                            mk &= mk - 1;
                            const float cs = __shfl(sv, src);
                            const int cj = wave * 32 + src;
                            const bool ins = wave_insert<uint32_t>(ls + cj * k, li + cj * k, k, cs, (uint32_t)row, lane);
                            changed |= ins && (fr == src);
                        }
                        thr_l = ls[jq * k + (k - 1)];
                    }
                }
                if (changed && fh == 0 && thr_l > thr_g) atomicMax(&gthr[q_base + jq], f2key(thr_l));
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        }
        if (pace_now && sib_lo + MF_LAG < (int)it) {
            int spin = 0;
            for (; spin < 2048 && sib_lo + MF_LAG < (int)it; ++spin) {
                __builtin_amdgcn_s_sleep(4);
                sib_lo = 1 << 30;
                for (int j = 0; j < nqtiles; ++j)
                    sib_lo = min(sib_lo, __hip_atomic_load(pace + (size_t)strip * nqtiles + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
            if (spin == 2048) pace = nullptr;   // a sibling is not running: stop waiting for it (thread 0's copy is the one used)
        }
        if (it + 1 < n_it) {
            MF_SSTORE(cur ^ 1)
        }
        __syncthreads();
        cur ^= 1;
        if (++kt == KT) {
            kt = 0;
            ++rt;
        }
    }
#undef MF_GLOAD
#undef MF_SSTORE
    // (a block that is done must not hold its siblings back)
    if (pace != nullptr && tid == 0)
        __hip_atomic_store(pace + (size_t)strip * nqtiles + qtile, 1 << 30, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // part layout: [q][strip][k]
    for (int i = tid; i < MF_BN * k; i += 256) {
        const int j = i / k, p = i - j * k;
        if (q_base + j < nq_real) {
            const size_t o = ((size_t)(q_base + j) * nstrips + strip) * k + p;
            part_s[o] = ls[i];
            part_i[o] = li[i];
        }
    }
}

// Split-bf16 variant of k_scan_mfma: every fp32 operand is split on the fly into a bf16 pair
// (h, l), x ~= h + l to 16 significant bits, and the four products (h+l).(h+l) run on
// v_mfma_f32_32x32x16_bf16 (16x the fp32-MFMA rate, 4 MFMAs instead of 8x2): ~4x the
// throughput at fp32-grade error (operand truncation 2^-17, random sign over 768 terms:
// ~1e-7 on unit vectors, same order as fp32 accumulation order effects).  The index stays
// fp32 in HBM; queries are pre-split once per search (k_split_queries).
// NW waves x 32 queries = BN query columns per block; every wave holds MT 32-row tiles (BM = 32*MT rows).
// (NW, MT) = (4, 4): 128x128 tile, <= 80 KiB LDS, two blocks per CU; (8, 8): 256x256 tile, one block of
// 8 waves per CU, half the operand bytes per MFMA (the CU's L2->LDS path is the scarce resource).
// The l_x.l_q product is <= 2^-18 |x.q| per term -- the size of the split's own truncation error -- and is
// not formed (three MFMAs per fp32-grade product instead of four).
constexpr bool kSplitLowLow = false;
template <int METRIC, int NW, int MT>
__global__ __launch_bounds__(64 * NW) void k_scan_mfma_split(const float* __restrict__ xb, const float* __restrict__ xnorm2,
                                                      const unsigned short* __restrict__ qsplit, int nq_real, int64_t ntotal,
                                                      int dpad, int k, int nstrips, int nqtiles,
                                                      int64_t tiles_per_strip, int* __restrict__ gthr,
                                                      float* __restrict__ part_s, uint32_t* __restrict__ part_i,
                                                      const uint32_t* __restrict__ mask) {
    constexpr int NT = 64 * NW, BM = 32 * MT, BN = 32 * NW;
    constexpr int APASS = BM * 4 / NT;   // A staging passes (rows per pass = NT/4)
    static_assert(NW <= MT && APASS >= 1, "tile shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* As = reinterpret_cast<float*>(smem);                 // [2][BM][32]
    float* Bs = As + 2 * BM * MF_BK;                         // [2][BM][32]
    float* xn2s = Bs + 2 * BN * MF_BK;                       // [BM]
    int* eflag = reinterpret_cast<int*>(xn2s + BM);          // [2] slow-path votes (alternating)
    float* ls = xn2s + BM + 4;                               // [BM][k]
    uint32_t* li = reinterpret_cast<uint32_t*>(ls + BN * k);  // [BM][k]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware decode: blocks l, l+8, l+16, ... (same XCD under round-robin dispatch)
    // walk the query tiles of ONE strip, so the strip's rows are fetched once per XCD L2.
    const int l = blockIdx.x;
    const int strip = (l / (8 * nqtiles)) * 8 + (l & 7);
    const int qtile = (l >> 3) % nqtiles;
    const int64_t ntiles = (ntotal + BM - 1) / BM;
    const int64_t t_begin = (int64_t)strip * tiles_per_strip;
    const int64_t t_end = min(t_begin + tiles_per_strip, ntiles);
    const int q_base = qtile * BN;

    for (int i = tid; i < BN * k; i += NT) {
        ls[i] = -INFINITY;
        li[i] = kInvalidRow;
    }
    if (tid < 2) eflag[tid] = 0;
    __syncthreads();
    if (t_begin >= t_end) {
        for (int i = tid; i < BN * k; i += NT) {
            const int j = i / k, p = i - j * k;
            if (q_base + j < nq_real) {
                const size_t o = ((size_t)(q_base + j) * nstrips + strip) * k + p;
                part_s[o] = -INFINITY;
                part_i[o] = kInvalidRow;
            }
        }
        return;
    }

    const int KT = dpad / MF_BK;
    const int64_t n_it = (t_end - t_begin) * KT;
    // staging map: thread -> (row = (tid>>3) + 32*i, 16-B chunk = tid&7), i = 0..3
    const int srow = tid >> 3, schunk = tid & 7;
    const int arow = tid >> 2, akg = tid & 3;
    // global loads run two K-steps ahead in two register sets when one wave per SIMD must hide the
    // whole L2/HBM latency (NW = 4); with two waves per SIMD (NW = 8) one set is enough and the
    // freed registers let the compiler read LDS fragments ahead of the MFMAs
    constexpr bool PF2 = NW < 8;
    v4f ra0[2 * APASS], rb0[4], ra1[PF2 ? 2 * APASS : 1], rb1[PF2 ? 4 : 1];

// (macros, not lambdas: by-reference lambda captures left ra/rb in scratch memory)
// A: thread -> row (tid>>2) + 64*i, 8 consecutive k = (tid&3)*8 (two float4), converted here to
// the bf16 pair (h, l) with x ~= h + l (16 significant bits); LDS row = [h k0..31 | l k0..31].
// B: the pre-split queries are copied 16 B at a time (thread -> row (tid>>3) + 32*i, chunk tid&7).
#define MF_GLOAD(RT, KT, RA, RB)                                                                                   \
    _Pragma("unroll") for (int i = 0; i < APASS; ++i) {                                                      \
        int64_t row_ = (RT) * BM + arow + (NT / 4) * i;                                                         \
        row_ = row_ < ntotal ? row_ : ntotal - 1;                                                            \
        const float* p_ = xb + row_ * (int64_t)dpad + (KT) * MF_BK + akg * 8;                                \
        RA[2 * i] = *reinterpret_cast<const v4f*>(p_);                                                       \
        RA[2 * i + 1] = *reinterpret_cast<const v4f*>(p_ + 4);                                               \
    }                                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        RB[i] = *reinterpret_cast<const v4f*>(qsplit + ((int64_t)(q_base + srow + (NT / 8) * i) * (dpad / MF_BK) + (KT)) * 64 + \
                                              schunk * 8);                                                   \
    }
#define MF_SSTORE(BUF, RA, RB)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < APASS; ++i) {                                                      \
        v8bf h_, l_;                                                                                         \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                      \
            const float x_ = j < 4 ? RA[2 * i][j] : RA[2 * i + 1][j - 4];                                    \
            const __bf16 hb_ = (__bf16)x_;                                                                   \
            h_[j] = hb_;                                                                                     \
            l_[j] = (__bf16)(x_ - (float)hb_);                                                               \
        }                                                                                                    \
        char* A_ = reinterpret_cast<char*>(As + (BUF) * BM * MF_BK);                                      \
        *reinterpret_cast<v8bf*>(A_ + mf_swz(arow + (NT / 4) * i, akg) * 4) = h_;                                  \
        *reinterpret_cast<v8bf*>(A_ + mf_swz(arow + (NT / 4) * i, 4 + akg) * 4) = l_;                              \
    }                                                                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                          \
        *reinterpret_cast<v4f*>(Bs + (BUF) * BN * MF_BK + mf_swz(srow + (NT / 8) * i, schunk)) = RB[i];         \
    }

    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    const int fr = lane & 31, fh = lane >> 5;
    const int jq = wave * 32 + fr;  // this lane's query column inside the tile
    float thr_g = -INFINITY;

    // software pipeline: global loads run TWO K-steps ahead in two register sets (one K-step of
    // MFMAs is shorter than the L2/HBM latency), LDS is double buffered one step ahead.
    int64_t rt = t_begin;  // row tile / K-step of the tile being computed
    int kt = 0;
    int64_t lrt = t_begin;  // (row tile, K-step) of the next global load to issue
    int lkt = 0;
#define MF_ADVANCE_LOAD()   \
    if (++lkt == KT) {      \
        lkt = 0;            \
        ++lrt;              \
    }
    MF_GLOAD(lrt, lkt, ra0, rb0)
    MF_ADVANCE_LOAD()
    MF_SSTORE(0, ra0, rb0)
    if (n_it > 1) {
        MF_GLOAD(lrt, lkt, ra0, rb0)  // tile 1 (PF2: set 0 again, tile 2 goes to set 1 below)
        MF_ADVANCE_LOAD()
    }
    if constexpr (PF2) {
        if (n_it > 2) {
            MF_GLOAD(lrt, lkt, ra1, rb1)
            MF_ADVANCE_LOAD()
        }
    }
    __syncthreads();
    int cur = 0;
// PF2 step: compute tile it | store tile it+1 (set RA/RB) to LDS | reload that set with tile it+3
#define MF_STEP2(RA, RB)                                                                   \
    {                                                                                      \
        MF_COMPUTE_AND_EPILOGUE()                                                          \
        if (it + 1 < n_it) {                                                               \
            MF_SSTORE(cur ^ 1, RA, RB)                                                     \
        }                                                                                  \
        if (it + 3 < n_it) {                                                               \
            MF_GLOAD(lrt, lkt, RA, RB)                                                     \
            MF_ADVANCE_LOAD()                                                              \
        }                                                                                  \
        __syncthreads();                                                                   \
        cur ^= 1;                                                                          \
        if (++kt == KT) {                                                                  \
            kt = 0;                                                                        \
            ++rt;                                                                          \
        }                                                                                  \
        ++it;                                                                              \
    }
// single-set step: compute tile it | store tile it+1 | load tile it+2 into the same set
#define MF_STEP1()                                                                         \
    {                                                                                      \
        MF_COMPUTE_AND_EPILOGUE()                                                          \
        if (it + 1 < n_it) {                                                               \
            MF_SSTORE(cur ^ 1, ra0, rb0)                                                   \
        }                                                                                  \
        if (it + 2 < n_it) {                                                               \
            MF_GLOAD(lrt, lkt, ra0, rb0)                                                   \
            MF_ADVANCE_LOAD()                                                              \
        }                                                                                  \
        __syncthreads();                                                                   \
        cur ^= 1;                                                                          \
        if (++kt == KT) {                                                                  \
            kt = 0;                                                                        \
            ++rt;                                                                          \
        }                                                                                  \
        ++it;                                                                              \
    }
    auto compute_and_epilogue = [&]() {
        const float* A = As + cur * BM * MF_BK;
        const float* B = Bs + cur * BN * MF_BK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {  // two 16-wide k-steps per 32-k tile; lane half fh takes chunk 2ks+fh
            const v8bf bh = *reinterpret_cast<const v8bf*>(B + mf_swz(jq, 2 * ks + fh));
            const v8bf bl = *reinterpret_cast<const v8bf*>(B + mf_swz(jq, 4 + 2 * ks + fh));
            // A fragments are read one 32-row tile ahead of the MFMAs that consume them, so the
            // LDS latency hides behind the previous tile's four MFMAs.
            v8bf ah_n = *reinterpret_cast<const v8bf*>(A + mf_swz(fr, 2 * ks + fh));
            v8bf al_n = *reinterpret_cast<const v8bf*>(A + mf_swz(fr, 4 + 2 * ks + fh));
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const v8bf ah = ah_n, al = al_n;
                if (m + 1 < MT) {
                    ah_n = *reinterpret_cast<const v8bf*>(A + mf_swz(32 * (m + 1) + fr, 2 * ks + fh));
                    al_n = *reinterpret_cast<const v8bf*>(A + mf_swz(32 * (m + 1) + fr, 4 + 2 * ks + fh));
                }
                // (h_x + l_x).(h_q + l_q): small terms first
                if constexpr (kSplitLowLow) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bl, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[m], 0, 0, 0);
            }
        }
        if (kt == KT - 1) {
            // ---------------- epilogue of row tile rt ----------------
            const int64_t row0 = rt * BM;
            if constexpr (METRIC == CSS_METRIC_L2) {
                // s = 2 x.q - ||x||^2  (||q||^2 is added in the final merge)
                if (tid < BM) xn2s[tid] = row0 + tid < ntotal ? xnorm2[row0 + tid] : 0.f;
                __syncthreads();
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[m][r] = 2.f * acc[m][r] - xn2s[32 * m + (r & 3) + 8 * (r >> 2) + 4 * fh];
            }
            thr_g = key2f(__hip_atomic_load(&gthr[q_base + jq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            float thr_l = ls[jq * k + (k - 1)];
            const float thr = fmaxf(thr_l, thr_g);
            const bool full_tile = row0 + BM <= ntotal;
            const bool colok = jq + q_base < nq_real;
            unsigned hitm = 0;  // bit m: this lane's query has a candidate in 32-row tile m
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                bool h = false;
#pragma unroll
                for (int r = 0; r < 16; ++r) h |= acc[m][r] >= thr;
                hitm |= (h && colok) ? (1u << m) : 0u;
            }
            const bool anyp = hitm != 0;
            // Block-uniform vote (one extra barrier per row tile): the slow path borrows the
            // just-consumed A staging buffer as its scratch, which keeps the block under 80 KiB
            // of LDS (two blocks per CU: one block's MFMAs overlap the other's staging).
            int* fl = eflag + (int)(rt & 1);
            if (__ballot(anyp) != 0ull && lane == 0) *fl = 1;
            __syncthreads();
            if (*fl) {
                if (tid == 0) eflag[(int)((rt + 1) & 1)] = 0;  // re-arm the other flag for the next row tile
                float* S = const_cast<float*>(As + cur * BM * MF_BK) + wave * (32 * 32);
                bool changed = false;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (__ballot((hitm >> m) & 1u) == 0ull) continue;  // wave-uniform: no candidate in this 32-row tile
#pragma unroll
                    for (int r = 0; r < 16; ++r) S[((r & 3) + 8 * (r >> 2) + 4 * fh) * 32 + fr] = acc[m][r];
                    for (int rr = 0; rr < 32; ++rr) {
                        const int64_t row = row0 + 32 * m + rr;
                        const float sv = S[rr * 32 + fr];
                        const bool pass = fh == 0 && (full_tile || row < ntotal) && q_base + jq < nq_real &&
                                          (mask == nullptr || ((mask[row >> 5] >> (row & 31)) & 1u)) &&
                                          sv >= thr_l && sv >= thr_g;
                        unsigned long long mk = __ballot(pass);
                        if (mk == 0ull) continue;
                        while (mk) {
                            const int src = __ffsll((long long)mk) - 1;
                            mk &= mk - 1;
                            const float cs = __shfl(sv, src);
                            const int cj = wave * 32 + src;
                            const bool ins = wave_insert<uint32_t>(ls + cj * k, li + cj * k, k, cs, (uint32_t)row, lane);
                            changed |= ins && (fr == src);
                        }
                        thr_l = ls[jq * k + (k - 1)];
                    }
                }
                if (changed && fh == 0 && thr_l > thr_g) atomicMax(&gthr[q_base + jq], f2key(thr_l));
            } else if (tid == 0) {
                eflag[(int)((rt + 1) & 1)] = 0;
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        }

    };
#define MF_COMPUTE_AND_EPILOGUE() compute_and_epilogue();
    // Invariant at the top of step `it`: LDS buf[cur] holds tile it; register set S(it+1) holds tile
    // it+1 (already loaded); PF2: set S(it+2) holds tile it+2.  S alternates 0,1 for PF2, is always 0 otherwise.
    if constexpr (PF2) {
        for (int64_t it = 0; it < n_it;) {
            // tile it+1 is in set 0 when `it` is even; tile it+3 is loaded into that set after it is stored
            MF_STEP2(ra0, rb0)
            if (it >= n_it) break;
            MF_STEP2(ra1, rb1)
        }
    } else {
        for (int64_t it = 0; it < n_it;) {
            MF_STEP1()
        }
    }
#undef MF_STEP1
#undef MF_STEP2
#undef MF_ADVANCE_LOAD
#undef MF_COMPUTE_AND_EPILOGUE
#undef MF_GLOAD
#undef MF_SSTORE
    // part layout: [q][strip][k]
    for (int i = tid; i < BN * k; i += NT) {
        const int j = i / k, p = i - j * k;
        if (q_base + j < nq_real) {
            const size_t o = ((size_t)(q_base + j) * nstrips + strip) * k + p;
            part_s[o] = ls[i];
            part_i[o] = li[i];
        }
    }
}



#include "css_knn_coarse.h"

// qpad [nq_pad][dpad] fp32 -> qsplit [nq_pad][dpad/32][h(32) | l(32)] bf16
__global__ void k_split_queries(const float* __restrict__ qpad, unsigned short* __restrict__ qsplit, int64_t n, int dpad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // element index
    if (i >= n * dpad) return;
    const int64_t row = i / dpad;
    const int c = (int)(i - row * dpad), kt = c >> 5, kk = c & 31;
    const float x = qpad[i];
    const __bf16 h = (__bf16)x;
    const __bf16 l = (__bf16)(x - (float)h);
    unsigned short* o = qsplit + (row * (dpad >> 5) + kt) * 64;
    o[kk] = __builtin_bit_cast(unsigned short, h);
    o[32 + kk] = __builtin_bit_cast(unsigned short, l);
}

// ------------------------------------------------------------------ final merge
// One block per query merges the G per-block lists (each sorted best-first) into
// the final top-k, RANK-MAJOR: round r looks at rank r of every list that is still
// alive.  A list whose rank-r entry cannot enter the current top-k is dead for
// good (its later ranks are worse and the k-th best only improves), so after the
// first round only a handful of lists stay alive.  Round 0 (all G heads) is a
// block-wide bitonic sort in LDS; later rounds append the few survivors to an LDS
// buffer and wave 0 inserts them.  G > 2048 is handled in chunks of 2048 lists.
constexpr int kMergeCap = 2048;
constexpr int kMergePerThread = kMergeCap / 256;
template <int METRIC>
__global__ __launch_bounds__(256) void k_merge_final(const float* __restrict__ part_s,
                                                     const uint32_t* __restrict__ part_i, int G, int k,
                                                     const int* __restrict__ gthr, const float* __restrict__ qnorm2,
                                                     int64_t id_base, float* __restrict__ D, int64_t* __restrict__ I,
                                                     int l2_expanded, float* __restrict__ cs_out,
                                                     uint32_t* __restrict__ ci_out, int* __restrict__ cn_out) {
    __shared__ float fs[CSS_KERNEL_MAX_K];
    __shared__ uint32_t fi[CSS_KERNEL_MAX_K];
    __shared__ float cs[kMergeCap];
    __shared__ uint32_t ci[kMergeCap];
    __shared__ int cnt;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)q * G * k;
    const float gfloor = key2f(gthr[q]);  // valid lower bound of the global k-th best
    for (int i = tid; i < k; i += 256) {
        fs[i] = -INFINITY;
        fi[i] = kInvalidRow;
    }
    __syncthreads();
    for (int c0 = 0; c0 < G; c0 += kMergeCap) {
        const int nb = min(kMergeCap, G - c0);  // lists in this chunk
        bool alive[kMergePerThread];
#pragma unroll
        for (int j = 0; j < kMergePerThread; ++j) alive[j] = tid + 256 * j < nb;
        int r0 = 0;
        if (c0 == 0) {
            // round 0: bitonic sort (best first) of the nb heads, padded to a power of two
            int n2 = 1;
            while (n2 < nb) n2 <<= 1;
            n2 = max(n2, 256);
            for (int i = tid; i < n2; i += 256) {
                float sv = -INFINITY;
                uint32_t iv = kInvalidRow;
                if (i < nb) {
                    const size_t o = base + (size_t)(c0 + i) * k;
                    const uint32_t id = part_i[o];
                    const float v = part_s[o];
                    if (id != kInvalidRow && v >= gfloor) {
                        sv = v;
                        iv = id;
                    }
                }
                cs[i] = sv;
                ci[i] = iv;
            }
            __syncthreads();
            for (int sz = 2; sz <= n2; sz <<= 1)
                for (int st = sz >> 1; st > 0; st >>= 1) {
                    for (int t = tid; t < n2 / 2; t += 256) {
                        const int lo = 2 * t - (t & (st - 1));  // index with bit `st` clear
                        const int hi = lo + st;
                        const bool desc = (lo & sz) == 0;      // best-first in the first half of each block
                        const float a = cs[lo], b2 = cs[hi];
                        const uint32_t ia = ci[lo], ib = ci[hi];
                        const bool a_first = better<uint32_t>(a, ia, b2, ib);
                        if (a_first != desc) {
                            cs[lo] = b2; ci[lo] = ib;
                            cs[hi] = a;  ci[hi] = ia;
                        }
                    }
                    __syncthreads();
                }
            for (int i = tid; i < k; i += 256) {
                fs[i] = cs[i];   // n2 >= 256 >= k
                fi[i] = ci[i];
            }
            __syncthreads();
            // a head that did not make the top-k kills its list
            const float kth = fs[k - 1];
            const uint32_t kid = fi[k - 1];
#pragma unroll
            for (int j = 0; j < kMergePerThread; ++j) {
                if (!alive[j]) continue;
                const size_t o = base + (size_t)(c0 + tid + 256 * j) * k;
                const uint32_t id = part_i[o];
                const float v = part_s[o];
                // alive iff the head is in the list, i.e. not worse than the k-th entry
                alive[j] = id != kInvalidRow && v >= gfloor && !better<uint32_t>(kth, kid, v, id);
            }
            r0 = 1;
            __syncthreads();
        }
        for (int r = r0; r < k; ++r) {
            if (tid == 0) cnt = 0;
            __syncthreads();
            const float kth = fs[k - 1];
            const uint32_t kid = fi[k - 1];
#pragma unroll
            for (int j = 0; j < kMergePerThread; ++j) {
                if (!alive[j]) continue;
                const size_t o = base + (size_t)(c0 + tid + 256 * j) * k + r;
                const uint32_t id = part_i[o];
                const float v = part_s[o];
                if (id != kInvalidRow && v >= gfloor && better<uint32_t>(v, id, kth, kid)) {
                    const int p = atomicAdd(&cnt, 1);
                    cs[p] = v;
                    ci[p] = id;
                } else {
                    alive[j] = false;
                }
            }
            __syncthreads();
            const int n = cnt;
            if (n == 0) break;  // block-uniform
            if (wave == 0)
                for (int c = 0; c < n; ++c) wave_insert<uint32_t>(fs, fi, k, cs[c], ci[c], lane);
            __syncthreads();
        }
        __syncthreads();
    }
    if (cs_out != nullptr) {
        // candidate-path caller (launch_scan_split_rescore): the k best scan scores, in the scan's own form, become
        // the query's candidate buffer for k_coarse_select<FINAL>
        for (int i = tid; i < k; i += 256) {
            const uint32_t id = fi[i];
            cs_out[(size_t)q * CZ_CAP + i] = id == kInvalidRow ? -INFINITY : fs[i];
            ci_out[(size_t)q * CZ_CAP + i] = id;
        }
        if (tid == 0) cn_out[(size_t)q * CZ_NS] = k;
        return;
    }
    for (int i = tid; i < k; i += 256) {
        const uint32_t id = fi[i];
        float s = fs[i];
        float d;
        if (METRIC == CSS_METRIC_IP) {
            d = id == kInvalidRow ? -FLT_MAX : s;
        } else {
            // scan kernels produce s = -(squared distance) (direct form) or, in the
            // expanded MFMA form, s = 2 x.q - ||x||^2 (||q||^2 added here)
            if (id == kInvalidRow) d = FLT_MAX;
            else if (l2_expanded) d = fmaxf(0.f, qnorm2[q] - s);
            else d = -s;
        }
        D[(size_t)q * k + i] = d;
        I[(size_t)q * k + i] = id == kInvalidRow ? (int64_t)-1 : id_base + (int64_t)id;
    }
}

// Merge of per-shard final results with global int64 ids (multi-GPU exchange).
// Part p holds its [nq, k] scores at Dp + p * stride_d and its ids at Ip + p * stride_i (elements): dense
// [nparts, nq, k] arrays, or the packed exchange records of the sharded search ([ids | scores] per rank).
template <int METRIC>
__global__ __launch_bounds__(64) void k_merge_parts(const float* __restrict__ Dp, const int64_t* __restrict__ Ip,
                                                    int nparts, int64_t stride_d, int64_t stride_i, int64_t nq, int k,
                                                    float* __restrict__ D, int64_t* __restrict__ I) {
    __shared__ float fs[CSS_KERNEL_MAX_K];
    __shared__ int64_t fi[CSS_KERNEL_MAX_K];
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    for (int i = lane; i < k; i += 64) {
        fs[i] = -INFINITY;
        fi[i] = INT64_MAX;
    }
    for (int p = 0; p < nparts; ++p)
        for (int j = 0; j < k; ++j) {
            const size_t o = (size_t)q * k + j;
            const int64_t id = Ip[(size_t)p * stride_i + o];
            if (id < 0) continue;  // wave uniform
            float s = Dp[(size_t)p * stride_d + o];
            if (METRIC == CSS_METRIC_L2) s = -s;
            wave_insert<int64_t>(fs, fi, k, s, id, lane);
        }
    for (int i = lane; i < k; i += 64) {
        const int64_t id = fi[i];
        const bool empty = id == INT64_MAX;
        float s = fs[i];
        D[q * k + i] = METRIC == CSS_METRIC_IP ? (empty ? -FLT_MAX : s) : (empty ? FLT_MAX : -s);
        I[q * k + i] = empty ? -1 : id;
    }
}

// ---- k beyond CSS_KERNEL_MAX_K (the reference passes k' = min(max_results, ntotal) for any max_results,
// src/storage.py:432): passes of up to CSS_KERNEL_MAX_K results per query, every pass over the rows the earlier
// passes did not return (an exclusion bitmap ANDed with the caller's allow-bitmap), then one sort of the k results.
__global__ void k_mask_init(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) dst[i] = src ? src[i] : 0xFFFFFFFFu;
}
__global__ void k_mask_clear(uint32_t* __restrict__ mask, const int64_t* __restrict__ I, int n, int64_t id_base) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = I[i] - id_base;
    if (I[i] >= 0 && r >= 0) atomicAnd(&mask[r >> 5], ~(1u << (r & 31)));
}
// one block per query: bitonic sort of its k (score, id) pairs by (score better first, lower id first; pads last)
template <int METRIC>
__global__ __launch_bounds__(1024) void k_sort_rows(float* __restrict__ D, int64_t* __restrict__ I, int k) {
    __shared__ float ss[CSS_MAX_K];
    __shared__ int64_t si[CSS_MAX_K];
    float* Dq = D + (size_t)blockIdx.x * k;
    int64_t* Iq = I + (size_t)blockIdx.x * k;
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        const bool real = i < k && Iq[i] >= 0;
        const float d = real ? Dq[i] : 0.f;
        ss[i] = real ? (METRIC == CSS_METRIC_IP ? d : -d) : -INFINITY;   // larger = better
        si[i] = real ? Iq[i] : INT64_MAX;
    }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n2 / 2; t += blockDim.x) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;   // this sub-sequence sorts best-first
                const float a = ss[lo], b = ss[hi];
                const int64_t ia = si[lo], ib = si[hi];
                const bool b_better = b > a || (b == a && ib < ia);
                if (b_better == up) {
                    ss[lo] = b; ss[hi] = a;
                    si[lo] = ib; si[hi] = ia;
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const bool empty = si[i] == INT64_MAX;
        Dq[i] = empty ? (METRIC == CSS_METRIC_IP ? -FLT_MAX : FLT_MAX) : (METRIC == CSS_METRIC_IP ? ss[i] : -ss[i]);
        Iq[i] = empty ? -1 : si[i];
    }
}

// The same merge for k beyond CSS_KERNEL_MAX_K (wave_insert holds two list slots per lane): every part is a list sorted
// by the total order (score better first, then lower id), ids are unique over the parts, so the final rank of entry j
// of part p is j + the number of entries of the other parts that precede it -- one binary search per other part.
template <int METRIC>
__global__ __launch_bounds__(256) void k_merge_parts_rank(const float* __restrict__ Dp, const int64_t* __restrict__ Ip,
                                                         int nparts, int64_t stride_d, int64_t stride_i, int64_t nq, int k,
                                                         float* __restrict__ D, int64_t* __restrict__ I) {
    const int64_t q = blockIdx.x;
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        D[q * k + i] = METRIC == CSS_METRIC_IP ? -FLT_MAX : FLT_MAX;
        I[q * k + i] = -1;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nparts * k; e += blockDim.x) {
        const int p = e / k, j = e - p * k;
        const size_t o = (size_t)q * k + j;
        const int64_t id = Ip[(size_t)p * stride_i + o];
        if (id < 0) continue;
        const float d = Dp[(size_t)p * stride_d + o];
        const float sc = METRIC == CSS_METRIC_IP ? d : -d;
        int rank = j;
        for (int p2 = 0; p2 < nparts && rank < k; ++p2) {
            if (p2 == p) continue;
            const float* D2 = Dp + (size_t)p2 * stride_d + (size_t)q * k;
            const int64_t* I2 = Ip + (size_t)p2 * stride_i + (size_t)q * k;
            int lo = 0, hi = k;   // first position of part p2 that does NOT precede (sc, id); pads precede nothing
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int64_t id2 = I2[mid];
                const float d2 = D2[mid];
                const float s2 = METRIC == CSS_METRIC_IP ? d2 : -d2;
                const bool precedes = id2 >= 0 && better<int64_t>(s2, id2, sc, id);
                if (precedes) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            D[q * k + rank] = d;
            I[q * k + rank] = id;
        }
    }
}

__global__ void k_fill_int(int* p, int n, int v) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

#include "css_knn_group.h"
#include "css_knn_diverse.h"

// ---------------------------------------------------------------- host side
// bf16 shadow rows for the coarse scan: kept when the metric is inner product, rows are a whole number
// of 64-element K stages and fp32 + bf16 rows fit in 80 % of the HBM (CSS_KNN_SHADOW=0/1 overrides).
bool want_shadow(css_index* ix, int64_t ncap) {
    if (ix->shadow == 0) return false;
    if (ix->dpad % 64 != 0) return false;
    static const int env_policy = [] {
        const char* e = getenv("CSS_KNN_SHADOW");
        return (e && e[0] == '0') ? 0 : ((e && e[0] == '1') ? 1 : -1);
    }();
    const int policy = ix->shadow_policy >= 0 ? ix->shadow_policy : env_policy;
    if (policy == 0 || policy == 2) return false;   // (2: int8 rows only, want_i8_only)
    if (policy == 1) return true;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
    return (double)ncap * ix->dpad * 6.0 <= 0.8 * (double)tot;
}

// CSS_KNN_I8=0 switches every int8 row copy off (read once)
bool i8_rows_allowed() {
    static const bool on = [] {
        const char* e = getenv("CSS_KNN_I8");
        return !(e && e[0] == '0');
    }();
    return on;
}

// int8 rows for the 1..4-query sweep (k_sweep_coarse_i8): only next to bf16 shadow rows, rows of at most 1024
// elements (the fp32 accumulation term of the sweep's error bound, cz_eps) and 7 bytes per element within 80 % of the HBM.
bool want_i8(css_index* ix, int64_t ncap) {
    if (!i8_rows_allowed() || ix->dpad % 64 != 0 || ix->dpad > 1024) return false;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
    return (double)ncap * ix->dpad * 7.0 <= 0.8 * (double)tot;
}

// int8 rows WITHOUT bf16 rows (5 bytes per element): shards of ~38-46 M rows of 768 floats on a 288 GB GPU, where fp32 +
// bf16 rows no longer fit in 80 % of the HBM but fp32 + int8 rows do -- such an index otherwise re-converts its rows into
// scratch memory on every batched search (6.7 ms per 10 M rows).  Only where the int8 scan and sweep apply (inner
// product, rows a whole number of 256-element K-step pairs, at most 1024 elements); css_index_set_shadow(ix, 2) forces
// it (tests), policy 0 forbids every shadow copy.
bool want_i8_only(css_index* ix, int64_t ncap) {
    if (!i8_rows_allowed() || ix->metric != CSS_METRIC_IP || ix->dpad % 256 != 0 || ix->dpad > 1024) return false;
    if (ix->shadow_policy == 0) return false;
    if (ix->shadow_policy == 2) return true;
    if (ix->shadow_policy == 1) return false;   // "always bf16" that did not fit: nothing
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
    return (double)ncap * ix->dpad * 5.0 <= 0.8 * (double)tot;
}

// `dst` (a column's own buffer, or its successor) with room for `cap` rows, every one at the column's default; on the
// index's stream
int column_alloc(css_index* ix, const RowColumn& col, int64_t cap, DevBuf<int32_t>* dst) {
    const int rc = dst->grow_exact((size_t)cap, col.what);
    if (rc != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemsetAsync(dst->p, col.fill, (size_t)cap * sizeof(int32_t), ix->stream));
    return CSS_OK;
}

// (Re)allocate the row storage for exactly ncap rows, carrying the ntotal existing rows over.  The new arrays are
// owned here until the swap at the end (whatever returns early frees them), the old ones from there on.
int reallocate_rows(css_index* ix, int64_t ncap) {
    DevBuf<float> nxb, nn2, nx8s;
    DevBuf<unsigned short> nxh;
    DevBuf<unsigned char> nx8;
    DevBuf<int32_t> ncol[css_index::kColumns];
    const auto cols = ix->columns();
    int rc;
    if ((rc = nxb.grow_exact((size_t)ncap * ix->dpad, "hipMalloc(index rows)")) != CSS_OK) return rc;
    // a column only where it was set: all default, then the existing rows' values
    for (int c = 0; c < css_index::kColumns; ++c)
        if (cols[c]->words.p && (rc = column_alloc(ix, *cols[c], ncap, &ncol[c])) != CSS_OK) return rc;
    // +256: the coarse scan reads whole tiles of norms
    if ((rc = nn2.grow_exact((size_t)ncap + 256, "hipMalloc(index norms)")) != CSS_OK) return rc;
    // the shadow can only be carried over (or started on an empty index), never rebuilt here
    const bool can_shadow = ix->xh.p != nullptr || ix->ntotal == 0;
    // (+256 rows: k_scan_coarse8 reads whole 256-row tiles; scores of rows >= ntotal are masked)
    // no room: batched search falls back to the split-operand kernel
    if (can_shadow && want_shadow(ix, ncap)) (void)nxh.try_exact(((size_t)ncap + 256) * ix->dpad);
    // the int8 rows of the few-query sweep ride along with the bf16 ones when 7 bytes per element still fit
    const bool i8_only = !nxh.p && ((ix->x8.p != nullptr && ix->xh.p == nullptr) || ix->ntotal == 0) && want_i8_only(ix, ncap);
    if ((nxh.p && (ix->x8.p != nullptr || ix->ntotal == 0) && want_i8(ix, ncap)) || i8_only) {
        if (!nx8.try_exact(((size_t)ncap + 256) * ix->dpad) || !nx8s.try_exact((size_t)ncap + 256)) {
            (void)nx8.drop();
            (void)nx8s.drop();
        }
    }
    if (ix->ntotal > 0) {
        if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ingest_ev, 0));
        if (nx8.p) {
            CSS_HIP_TRY(hipMemcpyAsync(nx8.p, ix->x8.p, (size_t)ix->ntotal * ix->dpad, hipMemcpyDeviceToDevice, ix->stream));
            CSS_HIP_TRY(hipMemcpyAsync(nx8s.p, ix->x8s.p, (size_t)ix->ntotal * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
        }
        CSS_HIP_TRY(hipMemcpyAsync(nxb.p, ix->xb.p, (size_t)ix->ntotal * ix->dpad * sizeof(float),
                                   hipMemcpyDeviceToDevice, ix->stream));
        CSS_HIP_TRY(hipMemcpyAsync(nn2.p, ix->xnorm2.p, (size_t)ix->ntotal * sizeof(float), hipMemcpyDeviceToDevice,
                                   ix->stream));
        if (nxh.p)
            CSS_HIP_TRY(hipMemcpyAsync(nxh.p, ix->xh.p, (size_t)ix->ntotal * ix->dpad * sizeof(unsigned short),
                                       hipMemcpyDeviceToDevice, ix->stream));
        for (int c = 0; c < css_index::kColumns; ++c)
            if (ncol[c].p)
                CSS_HIP_TRY(hipMemcpyAsync(ncol[c].p, cols[c]->words.p, (size_t)ix->ntotal * sizeof(int32_t),
                                           hipMemcpyDeviceToDevice, ix->stream));
    }
    bool filled = false;   // (a column's default fill is the one thing an empty index has in flight)
    for (const auto& nc : ncol) filled |= nc.p != nullptr;
    if (ix->ntotal > 0 || filled) CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    for (int c = 0; c < css_index::kColumns; ++c) cols[c]->words.swap(ncol[c]);
    ix->xb.swap(nxb);
    ix->xnorm2.swap(nn2);
    ix->xh.swap(nxh);
    ix->x8.swap(nx8);
    ix->x8s.swap(nx8s);
    ix->shadow = ix->xh.p ? 1 : 0;
    ix->cap = ncap;
    return CSS_OK;
}

int ensure_capacity(css_index* ix, int64_t need) {
    if (need > ix->cap) {
        int64_t ncap = std::max<int64_t>(need, ix->cap + ix->cap / 2);
        return reallocate_rows(ix, std::max<int64_t>(ncap, 1024));
    }
    if (ix->ntotal == 0 && !ix->xh.p && ix->shadow < 0 && ix->cap > 0 && want_shadow(ix, ix->cap)) {
        // emptied index (css_index_reset): start a shadow again if there is room now
        (void)ix->xh.try_exact(((size_t)ix->cap + 256) * ix->dpad);
        ix->shadow = ix->xh.p ? 1 : 0;
        if (ix->xh.p && !ix->x8.p && want_i8(ix, ix->cap)) {   // (the int8 pair whole or not at all, as reallocate_rows)
            if (!ix->x8.try_exact(((size_t)ix->cap + 256) * ix->dpad) || !ix->x8s.try_exact((size_t)ix->cap + 256)) {
                (void)ix->x8.drop();
                (void)ix->x8s.drop();
            }
        }
    }
    return CSS_OK;
}

int ingest(css_index* ix, const float* x_dev, int64_t n, int normalize, bool synth, uint64_t seed,
           int64_t first_row, hipStream_t st) {
    // One wave per row: a dispatch carries at most 2^32 work-items, i.e. 2^26 rows -- beyond that the rows were silently
    // not written (found with an 80 M-row index on one GPU: every search ended in the exact sweep over garbage rows).
    // 2^24 rows (2^30 work-items) per launch.
    constexpr int64_t kRowsPerLaunch = 1ll << 24;
    for (int64_t c0 = 0; c0 < n; c0 += kRowsPerLaunch) {
        const int64_t nc = std::min<int64_t>(kRowsPerLaunch, n - c0);
        const int64_t r0 = ix->ntotal + c0;
        const unsigned blocks = (unsigned)((nc + 3) / 4);
        float* dst = ix->xb.p + (size_t)r0 * ix->dpad;
        float* n2 = ix->xnorm2.p + r0;
        unsigned short* dh = ix->xh.p ? ix->xh.p + (size_t)r0 * ix->dpad : nullptr;
        unsigned char* d8 = ix->x8.p ? ix->x8.p + (size_t)r0 * ix->dpad : nullptr;
        float* d8s = ix->x8.p ? ix->x8s.p + r0 : nullptr;
        // appended rows are at every column's default (the slots may hold the values of rows removed earlier)
        for (RowColumn* col : ix->columns())
            if (col->words.p) CSS_HIP_TRY(hipMemsetAsync(col->words.p + r0, col->fill, (size_t)nc * sizeof(int32_t), st));
        if (synth)
            hipLaunchKernelGGL(k_ingest_rows<true>, dim3(blocks), dim3(256), 0, st, nullptr, dst, n2, nc, ix->dim, ix->dpad,
                               normalize, seed, first_row + c0, dh, ix->maxn2.p, (float*)nullptr, d8, d8s);
        else
            hipLaunchKernelGGL(k_ingest_rows<false>, dim3(blocks), dim3(256), 0, st, x_dev + (size_t)c0 * ix->dim, dst, n2, nc,
                               ix->dim, ix->dpad, normalize, 0ull, 0ll, dh, ix->maxn2.p, (float*)nullptr, d8, d8s);
        CSS_LAUNCH_CHECK();
    }
    return CSS_OK;
}

// ---- environment switches (benchmark labels and forced test paths): read once, never written afterwards
struct KnnEnv {
    int batch_i8 = 1;           // CSS_KNN_SCAN=bf16 / i8: batches always scan the bf16 / the int8 shadow rows (1 = where it pays)
    bool sweep_i8 = true;       // CSS_KNN_SWEEP=bf16: 1..4 queries sweep the bf16 shadow rows even where int8 rows exist (A/B runs)
    int growth = 0;       // CSS_KNN_GROWTH=4|8|16: growth factor of the nested row sample (batched MFMA cascade); 0: by k
    int growth_sweep = 0;   // CSS_KNN_GROWTH_SWEEP=4|8|16: the same for the few-query sweep cascades (0 = by shape: launch_scan_coarse)
    int sweep_fused = 1;    // CSS_KNN_SWEEP_FUSED=0 / 2: the 1..4-query cascade never / always as ONE launch (k_sweep_cascade); 1 = where it pays
    int qreg = 1;           // CSS_KNN_QREG=0: the int8 batch scan's later stages on k_scan_coarse8 instead of k_scan_qreg_i8 (A/B runs)
    int qreg_min = 1024;    // CSS_KNN_QREG_MIN=<tile tasks>: stages with fewer (row tile, query tile) pairs stay on k_scan_coarse8 (two per block: measured, launch_scan_coarse)
    int sweep_mfma = 1;     // CSS_KNN_SWEEP_MFMA=0: 3..32 queries never take the int8-MFMA sweep (A/B runs); 2: at every index size (tests)
    int fs_spins = CZ_FS_SPINS;   // CSS_KNN_FS_SPINS=n: polls before a waiting wave of k_sweep_cascade gives up (tests: 0 = at once)
};
const KnnEnv& knn_env() {
    static const KnnEnv env = [] {
        KnnEnv e;
        if (const char* m = getenv("CSS_KNN_SWEEP")) e.sweep_i8 = strcmp(m, "bf16") != 0;
        if (const char* m = getenv("CSS_KNN_SCAN")) e.batch_i8 = strcmp(m, "bf16") == 0 ? 0 : (strcmp(m, "i8") == 0 ? 2 : 1);
        if (const char* m = getenv("CSS_KNN_GROWTH")) {
            const int v = atoi(m);
            e.growth = (v == 4 || v == 8 || v == 16) ? v : 0;
        }
        if (const char* m = getenv("CSS_KNN_GROWTH_SWEEP")) {
            const int v = atoi(m);
            e.growth_sweep = (v == 4 || v == 8 || v == 16) ? v : 0;
        }
        if (const char* m = getenv("CSS_KNN_SWEEP_FUSED")) e.sweep_fused = m[0] == '0' ? 0 : (m[0] == '2' ? 2 : 1);
        if (const char* m = getenv("CSS_KNN_FS_SPINS")) e.fs_spins = std::max(0, atoi(m));
        if (const char* m = getenv("CSS_KNN_QREG")) e.qreg = m[0] == '0' ? 0 : 1;
        if (const char* m = getenv("CSS_KNN_QREG_MIN")) e.qreg_min = std::max(0, atoi(m));
        if (const char* m = getenv("CSS_KNN_SWEEP_MFMA")) e.sweep_mfma = m[0] == '0' ? 0 : (m[0] == '2' ? 2 : 1);
        return e;
    }();
    return env;
}

// geometry of the exact fp32 sweep (k_scan_small) for this index and k
struct SweepGeom {
    int nq_sweep;   // queries per sweep that fit the kernel's LDS budget (1..16)
    int G;          // blocks
    int64_t gpb;    // row groups (of 4) per block
};

// what only k_scan_small<FIX> reads (launch_fixup); the plain sweep passes it empty
struct FixArgs {
    const int* flag_list = nullptr;   // the flagged queries
    const int* nflag = nullptr;       // their count; the blocks-done word sits behind it
    float* fix_s = nullptr;           // one global list and lock per query
    uint32_t* fix_i = nullptr;
    int* fix_lock = nullptr;
    float* D = nullptr;               // result rows of the chunk
    int64_t* I = nullptr;
};

// The host fan-out of the exact fp32 sweeps (k_scan_small, k_range_small, k_scan_prior, k_scan_examples, k_facet_small), once.
// sweep_variant: f(TT, METRIC) with TT from dpad (12: the unrolled 768-float row, 0: any) and METRIC from the index.
// sweep_slots: f(NQ) with the smallest NQ of 1 / 2 / 8 / 16 that holds nqc queries (an NQ=4 instantiation spills under
// hipcc 7.2; 3..8 share NQ=8).  The arguments are std::integral_constants: decltype(X)::value is a template argument.
template <int V>
using IntC = std::integral_constant<int, V>;
template <typename F>
int sweep_variant(const css_index* ix, F&& f) {
    const bool ip = ix->metric == CSS_METRIC_IP;
    if (ix->dpad == 768) return ip ? f(IntC<12>(), IntC<CSS_METRIC_IP>()) : f(IntC<12>(), IntC<CSS_METRIC_L2>());
    return ip ? f(IntC<0>(), IntC<CSS_METRIC_IP>()) : f(IntC<0>(), IntC<CSS_METRIC_L2>());
}
template <typename F>
int sweep_slots(int nqc, F&& f) {
    return nqc <= 1 ? f(IntC<1>()) : nqc <= 2 ? f(IntC<2>()) : nqc <= 8 ? f(IntC<8>()) : f(IntC<16>());
}
// The same for the sweeps of the candidate cascade (k_sweep_coarse, k_sweep_coarse_i8, k_sweep_mfma_i8, k_sweep_cascade).
// sweep_nq_slots: f(NQ) with the smallest NQ of 1 / 2 / 4 that holds nq queries.
// sweep_unrolled<TT768>: f(TT, MAIN) -- 768 columns get the kernel's unrolled variant (TT768 steps: 6, 3 or 12 by
// kernel) and the split into main stage or not; every other width TT = 0 and MAIN = false.
template <typename F>
int sweep_nq_slots(int nq, F&& f) {
    return nq <= 1 ? f(IntC<1>()) : nq <= 2 ? f(IntC<2>()) : f(IntC<4>());
}
template <int TT768, typename F>
int sweep_unrolled(const css_index* ix, bool main_stage, F&& f) {
    if (ix->dpad == 768) return main_stage ? f(IntC<TT768>(), std::true_type()) : f(IntC<TT768>(), std::false_type());
    return f(IntC<0>(), std::false_type());
}
// The same for the token kernels, whose instantiations are taken as const void* (the callers have checked the ranges).
// tok_dim: f(P) with the token width P = 32 / 64 / 96 / 128.  tok_variant: f(P, MT, NB) with MT = 1 .. 4 tiles of 16
// query tokens and NB = 0 (a raw store) / 1 / 2 / 4 bits of a bucket.
template <typename F>
const void* tok_dim(int P, F&& f) {
    return P == 32 ? f(IntC<32>()) : P == 64 ? f(IntC<64>()) : P == 96 ? f(IntC<96>()) : f(IntC<128>());
}
template <typename F>
const void* tok_variant(int P, int MT, int NB, F&& f) {
    return tok_dim(P, [&](auto p) {
        auto tiles = [&](auto nb) -> const void* {
            return MT == 1 ? f(p, IntC<1>(), nb) : MT == 2 ? f(p, IntC<2>(), nb) : MT == 3 ? f(p, IntC<3>(), nb) : f(p, IntC<4>(), nb);
        };
        return NB == 0 ? tiles(IntC<0>()) : NB == 1 ? tiles(IntC<1>()) : NB == 2 ? tiles(IntC<2>()) : tiles(IntC<4>());
    });
}

template <int NQ, int TT, int METRIC, bool FIX>
int launch_scan_small_t(css_index* ix, const Rows& rows, const float* qpad, int nq_real, int k, int* gthr, const SweepGeom& sg,
                        hipStream_t st, const FixArgs& fx) {
    const int T = ix->dpad / 64;
    const size_t lds = (size_t)NQ * ix->dpad * 4 + (size_t)NQ * k * 8 + NQ * 8 + (FIX ? (size_t)4 * k * 8 : 0);
    auto kern = k_scan_small<NQ, TT, METRIC, FIX>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    ProfScope ps(FIX ? "knn_fix_scan" : "knn_scan_small", st);
    hipLaunchKernelGGL(kern, dim3(sg.G), dim3(256), lds, st, (const float4*)rows.xb, qpad, rows.n, T, k, sg.gpb, gthr,
                       ix->part_s.p, ix->part_i.p, nq_real, rows.mask, fx.flag_list, fx.nflag, fx.fix_s, fx.fix_i, fx.fix_lock,
                       FIX ? const_cast<int*>(fx.nflag) + 1 : (int*)nullptr, rows.id_base, fx.D, fx.I);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int NQ, bool FIX>
int launch_scan_small_nq(css_index* ix, const Rows& rows, const float* qpad, int nq_real, int k, int* gthr, const SweepGeom& sg,
                         hipStream_t st, const FixArgs& fx = FixArgs()) {
    return sweep_variant(ix, [&](auto TT, auto M) {
        return launch_scan_small_t<NQ, decltype(TT)::value, decltype(M)::value, FIX>(ix, rows, qpad, nq_real, k, gthr, sg, st, fx);
    });
}

// the per-block top-k lists of the exact scans: [q][block][k] scores and rows
int grow_part(css_index* ix, size_t entries) {
    const int rc = ix->part_s.grow(entries, "hipMalloc(part_s)");
    return rc != CSS_OK ? rc : ix->part_i.grow(entries, "hipMalloc(part_i)");
}

inline int host_f2key(float f) {
    int i;
    memcpy(&i, &f, 4);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}

// (defined behind search_chunk_small, where the merge kernels were first used: the code object keeps its kernel order)
int launch_merge_final(css_index* ix, const Rows& rows, int q0, int nqc, int k, const SweepGeom& sg, float* D_dev,
                       int64_t* I_dev, hipStream_t st);

// Queries [q0, q0+nqc) (nqc <= 16) against the whole index, results to D/I rows q0...
int search_chunk_small(css_index* ix, const Rows& rows, int q0, int nqc, int k, const SweepGeom& sg, float* D_dev,
                       int64_t* I_dev, hipStream_t st) {
    int* gthr = ix->gthr.p + q0;
    hipLaunchKernelGGL(k_fill_int, dim3(1), dim3(64), 0, st, gthr, nqc, host_f2key(-INFINITY));
    CSS_LAUNCH_CHECK();
    const float* qp = ix->qpad.p + (size_t)q0 * ix->dpad;
    const int rc = sweep_slots(nqc, [&](auto NQ) {
        return launch_scan_small_nq<decltype(NQ)::value, false>(ix, rows, qp, nqc, k, gthr, sg, st);
    });
    return rc != CSS_OK ? rc : launch_merge_final(ix, rows, q0, nqc, k, sg, D_dev, I_dev, st);
}

// The plain merge behind a sweep: the [block][k] part lists of queries [q0, q0 + nqc) into D/I rows q0... (keys are
// "larger is better" for both metrics; <L2> writes D = -key)
int launch_merge_final(css_index* ix, const Rows& rows, int q0, int nqc, int k, const SweepGeom& sg, float* D_dev,
                       int64_t* I_dev, hipStream_t st) {
    ProfScope ps("knn_merge", st);
    const auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(nqc), dim3(256), 0, st, ix->part_s.p, ix->part_i.p, sg.G, k, ix->gthr.p + q0,
                           ix->qnorm2.p + q0, rows.id_base, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, 0, (float*)nullptr,
                           (uint32_t*)nullptr, (int*)nullptr);
    };
    if (ix->metric == CSS_METRIC_IP) go(k_merge_final<CSS_METRIC_IP>);
    else go(k_merge_final<CSS_METRIC_L2>);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Device-side exact fix-up of the queries a candidate path flagged (overflowing buffer or band, band not closed):
// one launch that returns at once when nothing is flagged (nflag[1]: its blocks-done counter, zeroed with the count).
// qpad, gthr, D_dev and I_dev are already offset to the chunk's first query; the flagging kernel has reset gthr / fix
// lists / locks of every flagged query.
int launch_fixup(css_index* ix, const Rows& rows, const float* qpad, int nq, int k, int* gthr, const int* flag_list,
                 const int* nflag, float* D_dev, int64_t* I_dev, const SweepGeom& sg, hipStream_t st) {
    const FixArgs fx{flag_list, nflag, ix->fix_s.p, ix->fix_i.p, ix->fix_lock.p, D_dev, I_dev};
    if (sg.nq_sweep >= 8) return launch_scan_small_nq<8, true>(ix, rows, qpad, 8, k, gthr, sg, st, fx);
    if (sg.nq_sweep >= 2) return launch_scan_small_nq<2, true>(ix, rows, qpad, 2, k, gthr, sg, st, fx);
    return launch_scan_small_nq<1, true>(ix, rows, qpad, 1, k, gthr, sg, st, fx);
}

// workspaces shared by the candidate paths: thresholds, candidate buffers, flags, fix-up lists for nq_pad queries
int grow_candidate_ws(css_index* ix, size_t nq_pad, int k) {
    int rc;
    if ((rc = ix->cthr.grow(nq_pad)) != CSS_OK) return rc;
    if ((rc = ix->cand_n.grow((size_t)nq_pad * CZ_NS)) != CSS_OK) return rc;
    if ((rc = ix->rs_work.grow(1 + (size_t)nq_pad * CZ_PARTS)) != CSS_OK) return rc;
    ix->last_nflag = nullptr;
    ix->last_nswept = nullptr;
    if ((rc = ix->cflags.grow(2 * nq_pad + 2)) != CSS_OK) return rc;
    if ((rc = ix->cand_s.grow(nq_pad * CZ_CAP)) != CSS_OK) return rc;
    if ((rc = ix->cand_i.grow(nq_pad * CZ_CAP)) != CSS_OK) return rc;
    if ((rc = ix->fix_lock.grow(nq_pad)) != CSS_OK) return rc;
    if ((rc = ix->fix_s.grow_exact(nq_pad * (size_t)k, "hipMalloc(fix_s)")) != CSS_OK) return rc;
    return ix->fix_i.grow_exact(nq_pad * (size_t)k, "hipMalloc(fix_i)");
}

// second coarse pass over flagged queries: slots (query rows) and candidates per slot
constexpr int kF2Max = 1024;
constexpr int CZ_CAP2 = 32768;
// largest k the MFMA kernels' LDS lists hold next to their staging buffers
constexpr int kMfmaMaxK = 64;
// extra ranks the split-operand candidate scan keeps beyond k (the band must close inside them, else the
// query is flagged and re-run exactly)
constexpr int kSplitExtra = 4;
// |split score - x.q| <= kSplitEps ||q|| max||x||: operand residuals 2 x 2^-16, the dropped l.l term 2^-16,
// 144 fp32 accumulation steps 2^-16.8 -- together < 3.6 x 2^-16; 2^-14 leaves a margin
constexpr float kSplitEps = 6.103515625e-05f;

// Exact fp32 batched scan (CSS_SEARCH_EXACT_FP32 with more than 16 queries):
// v_mfma_f32_32x32x2_f32, bit-exact fmaf chains, scores written as they are.
template <int METRIC>
int launch_scan_fp32mfma(css_index* ix, const Rows& rows, int nq, int k, float* D_dev, int64_t* I_dev, hipStream_t st) {
    const int nq_pad = (nq + MF_BN - 1) / MF_BN * MF_BN;  // <= nq + 127 (qpad / gthr have 256 rows of slack)
    const int nqtiles = nq_pad / MF_BN;
    const int64_t ntiles = (rows.n + MF_BM - 1) / MF_BM;
    const size_t lds = (size_t)(2 * MF_BM * MF_BK + 2 * MF_BN * MF_BK + 4 * 32 * 33 + MF_BM) * 4 + (size_t)MF_BN * k * 8;
    // strips in multiples of 8 for the XCD-aware block decode
    int nstrips = std::max(8, ix->num_cus / nqtiles / 8 * 8);
    nstrips = (int)std::min<int64_t>(nstrips, (ntiles + 7) / 8 * 8);
    const int64_t tps = (ntiles + nstrips - 1) / nstrips;
    int rc;
    if ((rc = grow_part(ix, (size_t)nq * nstrips * k)) != CSS_OK) return rc;
    if (nq_pad > nq)
        CSS_HIP_TRY(hipMemsetAsync(ix->qpad.p + (size_t)nq * ix->dpad, 0, (size_t)(nq_pad - nq) * ix->dpad * 4, st));
    hipLaunchKernelGGL(k_fill_int, dim3((nq_pad + 255) / 256), dim3(256), 0, st, ix->gthr.p, nq_pad, host_f2key(-INFINITY));
    CSS_LAUNCH_CHECK();
    auto kern = k_scan_mfma<METRIC>;
    if ((rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    // sibling pacing (see the kernel) where a strip has siblings; the counters share the cascade's pacing words
    int* pace = nullptr;
    if (nqtiles > 1 && nstrips * nqtiles <= ix->num_cus) {   // (all blocks resident: one per CU)
        if ((rc = ix->cpace.grow((size_t)nstrips * nqtiles)) != CSS_OK) return rc;
        pace = ix->cpace.p;
        CSS_HIP_TRY(hipMemsetAsync(pace, 0, (size_t)nstrips * nqtiles * sizeof(int), st));
    }
    {
        ProfScope ps("knn_scan_mfma", st);
        hipLaunchKernelGGL(kern, dim3(nstrips * nqtiles), dim3(256), lds, st, rows.xb, rows.xnorm2, ix->qpad.p, nq,
                           rows.n, ix->dpad, k, nstrips, nqtiles, tps, ix->gthr.p, ix->part_s.p, ix->part_i.p, rows.mask, pace);
        CSS_LAUNCH_CHECK();
    }
    {
        ProfScope ps("knn_merge", st);
        hipLaunchKernelGGL(k_merge_final<METRIC>, dim3(nq), dim3(256), 0, st, ix->part_s.p, ix->part_i.p, nstrips, k,
                           ix->gthr.p, ix->qnorm2.p, rows.id_base, D_dev, I_dev, METRIC == CSS_METRIC_L2 ? 1 : 0,
                           (float*)nullptr, (uint32_t*)nullptr, (int*)nullptr);
        CSS_LAUNCH_CHECK();
    }
    return CSS_OK;
}

// Batched candidate path of an index WITHOUT bf16 shadow rows (shards beyond ~38 M rows of 768 floats, or
// css_index_set_shadow(0)): the coarse scores are split-operand products formed from the fp32 rows
// (k_scan_mfma_split: h.h + h.l + l.h, error <= kSplitEps ||q|| max||x||), the scan keeps k + kSplitExtra
// ranks per query, and k_coarse_select<FINAL> rescores the band in fp32 exactly as the bf16 cascade does.  A
// query whose band does not close inside the kept ranks is flagged and re-run by the device-side fix-up.
// After the last stage of a candidate scan: band cut + flagging (one block per query), exact rescoring of the bands
// (CZ_PARTS work items per query over a fixed grid), sort by exact score + output (one block per query).
constexpr int kRescoreGrid = 4096;
struct EpsSet {   // what cz_eps needs to know about the operands a scan read
    float eps_rel;        // a-priori bound relative to ||q|| max||x||
    const float* qerr2;   // per query ||q - q^||^2 (null: fp32 queries)
    int measured;         // the word of maxn2 with the rows' measured error (1 bf16, 2 int8)
};
int launch_final_select(css_index* ix, const Rows& rows, int nq, int k, EpsSet e1, EpsSet e2, bool exact_k, int l2,
                        int closed_n, const float* qpad, const float* qnorm2, int* gthr, int* flags, int* nflag,
                        int* flag_list, float* D_dev, int64_t* I_dev, float* thr2, unsigned short* qh2, int f2,
                        hipStream_t st) {
    // e1: the scan that filled the buffers; e2: the second pass over flagged queries (always bf16 rows and queries)
    const float eps_rel = e1.eps_rel;
    const float* qerr2 = e1.qerr2;
    const int measured = e1.measured;
    hipLaunchKernelGGL(k_coarse_select<true>, dim3(nq), dim3(256), 0, st, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p, ix->cthr.p, flags,
                       nflag, flag_list, qnorm2, ix->maxn2.p, eps_rel, l2, k, closed_n, gthr, qerr2, measured, ix->fix_s.p, ix->fix_i.p, ix->fix_lock.p,
                       exact_k ? qpad : (const float*)nullptr, exact_k ? (const float*)rows.xb : (const float*)nullptr, ix->dpad);
    // (a work list of the live parts pays from a few dozen queries on; a handful of queries launch all their parts)
    const bool plan = nq > 16;
    if (plan) hipLaunchKernelGGL(k_rescore_plan, dim3(1), dim3(1024), 0, st, (const int*)ix->cand_n.p, nq, ix->rs_work.p, ix->rs_work.p + 1);
    hipLaunchKernelGGL(k_rescore_parts<false>, dim3(std::min(kRescoreGrid, nq * CZ_PARTS)), dim3(256), 0, st, ix->cand_s.p,
                       ix->cand_i.p, ix->cand_n.p, CZ_CAP, nq, (const int*)nullptr, (const int*)nullptr, (const float*)nullptr, l2, qpad,
                       rows.xb, ix->dpad, plan ? (const int*)ix->rs_work.p : (const int*)nullptr,
                       plan ? (const int*)(ix->rs_work.p + 1) : (const int*)nullptr);
    hipLaunchKernelGGL(k_coarse_final, dim3(nq), dim3(256), 0, st, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p, flags, qnorm2, ix->maxn2.p,
                       e2.eps_rel, l2, k, qpad, ix->dpad, rows.id_base, D_dev, I_dev, thr2, qh2, f2, e2.qerr2, e2.measured);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int METRIC>
int launch_scan_split_rescore(css_index* ix, const Rows& rows, int q0, int nq, int k, float* D_dev, int64_t* I_dev,
                              const SweepGeom& sg, hipStream_t st) {
    // queries [q0, q0 + nq) of the padded query rows; nq <= 4096 and q0 a multiple of 256 (the caller chunks: the
    // candidate buffers are 32 KiB per query, and only the last chunk has padding rows to clear)
    const int kp = k + kSplitExtra;
    float* const qpad = ix->qpad.p + (size_t)q0 * ix->dpad;
    float* const qnorm2 = ix->qnorm2.p + q0;
    int* const gthr = ix->gthr.p + q0;
    D_dev += (size_t)q0 * k;
    I_dev += (size_t)q0 * k;
    const bool big = nq > 128 && kp <= 14;  // 256x256 tiles (8 waves) for real batches
    const int BMs = big ? 256 : MF_BM, BNs = big ? 256 : MF_BN;
    const int nq_pad = (nq + BNs - 1) / BNs * BNs;  // <= nq + 255 (qpad / gthr have 256 rows of slack)
    const int nqtiles = nq_pad / BNs;
    const int64_t ntiles = (rows.n + BMs - 1) / BMs;
    // staging + lists (the slow-path scratch borrows a staging buffer); <= 80 KiB means two blocks share a CU
    const size_t lds = (size_t)(2 * BMs * MF_BK + 2 * BNs * MF_BK + BMs + 4) * 4 + (size_t)BNs * kp * 8;
    const int bpc = (!big && lds <= 80 * 1024) ? 2 : 1;
    int nstrips = std::max(8, bpc * ix->num_cus / nqtiles / 8 * 8);
    nstrips = (int)std::min<int64_t>(nstrips, (ntiles + 7) / 8 * 8);
    const int64_t tps = (ntiles + nstrips - 1) / nstrips;
    int rc;
    if ((rc = grow_part(ix, (size_t)nq * nstrips * kp)) != CSS_OK) return rc;
    if ((rc = grow_candidate_ws(ix, (size_t)nq_pad, k)) != CSS_OK) return rc;
    if ((rc = ix->qsplit.grow((size_t)nq_pad * ix->dpad * 2)) != CSS_OK) return rc;
    int* flags = ix->cflags.p;
    int* flag_list = ix->cflags.p + nq_pad;
    int* nflag = ix->cflags.p + 2 * nq_pad;
    ix->last_nflag = nflag;
    ix->last_nswept = nflag;
    if (nq_pad > nq)
        CSS_HIP_TRY(hipMemsetAsync(qpad + (size_t)nq * ix->dpad, 0, (size_t)(nq_pad - nq) * ix->dpad * 4, st));
    hipLaunchKernelGGL(k_fill_int, dim3((nq_pad + 255) / 256), dim3(256), 0, st, gthr, nq_pad, host_f2key(-INFINITY));
    hipLaunchKernelGGL(k_coarse_init, dim3((nq_pad + 255) / 256), dim3(256), 0, st, ix->cthr.p, ix->cand_n.p, flags, nflag,
                       nq, nq_pad, 0, (int*)nullptr, 0, (int*)nullptr, (float*)nullptr, (int*)nullptr, 0, (int*)nullptr,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, 0, 0, 0);
    const int64_t ne = (int64_t)nq_pad * ix->dpad;
    hipLaunchKernelGGL(k_split_queries, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, qpad, ix->qsplit.p,
                       (int64_t)nq_pad, ix->dpad);
    CSS_LAUNCH_CHECK();
    ProfScope all("knn_split_cascade", st);
    {
        ProfScope ps("knn_scan_split", st);
        if (big) {
            auto kern = k_scan_mfma_split<METRIC, 8, 8>;
            if ((rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
            hipLaunchKernelGGL(kern, dim3(nstrips * nqtiles), dim3(512), lds, st, rows.xb, rows.xnorm2, ix->qsplit.p, nq,
                               rows.n, ix->dpad, kp, nstrips, nqtiles, tps, gthr, ix->part_s.p, ix->part_i.p, rows.mask);
        } else {
            auto kern = k_scan_mfma_split<METRIC, 4, 4>;
            if ((rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
            hipLaunchKernelGGL(kern, dim3(nstrips * nqtiles), dim3(256), lds, st, rows.xb, rows.xnorm2, ix->qsplit.p, nq,
                               rows.n, ix->dpad, kp, nstrips, nqtiles, tps, gthr, ix->part_s.p, ix->part_i.p, rows.mask);
        }
        CSS_LAUNCH_CHECK();
    }
    // the kp best split scores of every query -> its candidate buffer (scores stay in the scan's form: IP dot
    // products, L2 2 x.q - ||x||^2, the form k_coarse_select expects of coarse scores)
    hipLaunchKernelGGL(k_merge_final<METRIC>, dim3(nq), dim3(256), 0, st, ix->part_s.p, ix->part_i.p, nstrips, kp, gthr,
                       qnorm2, rows.id_base, D_dev, I_dev, METRIC == CSS_METRIC_L2 ? 1 : 0, ix->cand_s.p, ix->cand_i.p,
                       ix->cand_n.p);
    if ((rc = launch_final_select(ix, rows, nq, k, EpsSet{kSplitEps, nullptr, 0}, EpsSet{kSplitEps, nullptr, 0}, false, METRIC == CSS_METRIC_L2 ? 1 : 0, kp, qpad, qnorm2, gthr, flags, nflag,
                                  flag_list, D_dev, I_dev, nullptr, nullptr, 0, st)) != CSS_OK)
        return rc;
    return launch_fixup(ix, rows, qpad, nq, k, gthr, flag_list, nflag, D_dev, I_dev, sg, st);
}

// Coarse bf16 scan + exact rescoring (css_knn_coarse.h) for queries [q0, q0 + nq) of ix->qpad.p; nq <= 4096.
template <int NQ, int TT, bool MAIN>
int launch_sweep_coarse_t(css_index* ix, const Rows& rows, const float* qpad, int nq, int64_t count, int64_t stride,
                          int gm1, bool stage0, hipStream_t st) {
    const size_t lds = (size_t)NQ * ix->dpad * sizeof(float);
    const int grid = (int)std::min<int64_t>((int64_t)ix->num_cus * 8, count);
    auto kern = k_sweep_coarse<NQ, TT, MAIN>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, rows.xh, qpad, ix->cthr.p, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p,
                       rows.n, ix->dpad, nq, count, stride, gm1, stage0 ? 1 : 0, rows.mask,
                       ix->metric == CSS_METRIC_L2 ? rows.xnorm2 : nullptr);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int NQ, int TT, bool MAIN>
int launch_sweep_coarse_i8_t(css_index* ix, const Rows& rows, const float* qpad, int nq, int64_t count, int64_t stride,
                             int gm1, bool stage0, hipStream_t st) {
    const int steps = TT > 0 ? TT : (ix->dpad / 16 + 15) / 16;
    const size_t lds = ((size_t)NQ * 256 * steps + NQ) * sizeof(float);
    const int grid = (int)std::min<int64_t>((int64_t)ix->num_cus * 8, count);
    auto kern = k_sweep_coarse_i8<NQ, TT, MAIN>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, rows.x8, rows.x8s, qpad, ix->cthr.p, ix->cand_s.p, ix->cand_i.p,
                       ix->cand_n.p, rows.n, ix->dpad, nq, count, stride, gm1, stage0 ? 1 : 0, rows.mask,
                       ix->metric == CSS_METRIC_L2 ? rows.xnorm2 : nullptr);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Rows whose int8 copy is poor (a few dominant elements set the row scale and the rest rounds to nothing) make the
// measured band so wide that the buffers overflow and the queries end in the fix-up: results stay exact, the search
// gets slow.  So the use of the int8 rows adapts per index: `permille` = flagged share of the last int8 search above
// which the next 16 searches of that kind read the bf16 rows, then int8 is tried again.  (Caller holds ws_mu.)
inline bool i8_feedback_allows(css_index::I8Feedback& f, int permille) {
    if (f.pending && hipEventQuery(f.ev) == hipSuccess) {
        f.pending = false;
        if ((int64_t)*f.h_nflag * 1000 > (int64_t)f.nq * permille) f.backoff = 16;
    }
    if (f.backoff > 0) {
        --f.backoff;
        return false;
    }
    return true;
}
inline int i8_feedback_record(css_index::I8Feedback& f, const int* nflag_dev, int nq, hipStream_t st) {
    if (f.h_nflag == nullptr) {
        CSS_HIP_TRY(hipHostMalloc((void**)&f.h_nflag, sizeof(int), hipHostMallocDefault));
        CSS_HIP_TRY(hipEventCreateWithFlags(&f.ev, hipEventDisableTiming));
    }
    if (!f.pending) {
        CSS_HIP_TRY(hipMemcpyAsync(f.h_nflag, nflag_dev, sizeof(int), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipEventRecord(f.ev, st));
        f.pending = true;
        f.nq = nq;
    }
    return CSS_OK;
}
// 1..4 queries: any flagged query sends the next searches back to the bf16 sweep
inline bool sweep_uses_i8(css_index* ix, const Rows& rows) {
    if (rows.x8 == nullptr || !knn_env().sweep_i8) return false;
    return i8_feedback_allows(ix->fb_sweep, 0);
}
// batches: the int8 MFMA scan -- inner product, rows a whole (even) number of 128-B K steps, the 8-phase loop's shape --
// where it pays: its candidate band is wider than the bf16 scan's (with the one-eps thresholds of k_coarse_select ~150
// instead of ~25 band rows per query at 10 M rows, all rescored exactly, and the k best candidates are scored exactly
// in every select), costs per query that do not shrink with the index, while the saving is half of the scan.
// Measured (1000 queries, ms int8 / bf16, one session): k = 10: 0.1 M rows 0.40 / 0.32, 0.2 M 0.57 / 0.49, 0.3 M
// 0.64 / 0.68, 0.6 M 0.93 / 1.06, 1 M 1.25 / 1.61, 1.25 M 1.42 / 1.95, 2.5 M 2.35 / 3.5, 10 M 7.6-7.8 / 12.3-13.1;
// 10 M rows: k = 16 7.8 / 12.6, k = 32 8.4 / 12.8, k = 64 9.7 / 13.3, k = 100 10.8 / 13.7, k = 128 11.6 / 14.0; but
// 1 M rows, k = 100: 3.0 / 2.2, and 64 queries, k = 100, 10 M rows: 3.8 / 3.6 (the selects score k rows per query
// exactly); 4096 queries, k = 10: 29.0 / 52.3.  CSS_KNN_SCAN=i8 / bf16 force one or the other.
// Its wider band also flags more queries on clustered rows (10 M rows in 20 000 clusters: 23 % of the queries, 14.8 ms
// against the bf16 scan's 13.3 with none flagged), so the choice adapts per index: when an int8 batch flagged more than
// 5 % of its queries the next 16 batches read the bf16 rows, then int8 is tried again.  (Caller holds ws_mu.)
// (`nrows`: the rows one cascade covers -- the index, or one range of a shadow-less index)
inline bool batch_i8_wanted(css_index* ix, int k, int64_t nrows, int64_t nq) {
    const KnnEnv& e = knn_env();
    if (e.batch_i8 == 0 || ix->metric != CSS_METRIC_IP || ix->dpad % 256 != 0 || ix->dpad > 1024) return false;
    if (e.batch_i8 == 2) return true;
    // (round 4, later stages on k_scan_qreg_i8, ms int8 / bf16: k = 100, 1000 queries: 4 M rows 4.1 / 6.1, 2 M 2.7 / 3.3, 1 M 2.0 /
    // 2.0, 300 k 1.3 / 0.9; 256 queries: 2 M 1.0 / 1.4, 1 M 0.87 / 0.75.  k = 10: 1 M 1.04 / 1.57, 300 k 0.53 / 0.64 (256 queries
    // 0.31 / 0.31), 100 k 0.35 / 0.31)
    // (fewer than 256 queries, k = 100, ms int8 / bf16, 33 / 64 / 128 / 255 queries: 10 M rows 1.89 / 3.19, 2.08 / 3.33, 2.19 /
    // 3.45, 2.50 / 3.87; 2 M rows 0.73 / 0.82 .. 0.99 / 1.08: the query count is no condition any more)
    (void)nq;
    const bool pays = k <= 32 ? nrows >= 300000 : (k * 2 <= CZ_EXK && nrows >= 2000000);
    if (!pays) return false;
    // (with <= 256 flagged queries the second pass is one query tile of bf16 scan -- a quarter of a 1000-query bf16 step --
    // and the int8 search still wins: 10 M rows in 20 000 clusters, 33 flagged: 12.8 ms against 13.3 on bf16 rows)
    return i8_feedback_allows(ix->fb_batch, 50);
}

// 3..32 queries, inner product, int8 rows in view: does the sweep on the int8 MFMA (k_sweep_mfma_i8) answer sooner than what
// it replaces -- the VALU sweep (3, 4 queries) or the 256-query tiles of the batch scan?  One
// session, ms with / without, 3 .. 16 queries: 10 M rows k = 10 1.65 / 1.92-2.07, k = 100 1.83-1.85 / 2.75-3.26; 1 M rows
// 0.32-0.33 / 0.34-0.41 and 0.46-0.48 / 0.45-0.58; 100 k rows 0.13-0.14 / 0.15-0.16 but 0.22 / 0.18-0.20 at k = 100 (a
// select with 100 exactly scored rows behind every stage); 20 k rows 0.11-0.12 / 0.11 and 0.17-0.19 / 0.13-0.15.
inline bool mfma_sweep_applies(const css_index* ix, const Rows& rows, int64_t nq, int k) {
    const int mode = knn_env().sweep_mfma;
    if (mode == 0 || rows.x8 == nullptr || ix->metric != CSS_METRIC_IP || ix->dpad > 1024 || nq < 3 || nq > 32) return false;
    if (mode == 2) return true;
    // 17..32 queries (two fragment sets per lane), ms with / without: k = 10: 10 M rows 1.78 / 1.66 (the batch scan with the
    // queries in registers is ahead there), 1 M rows 0.33 / 0.38, 100 k rows 0.13 / 0.155; k = 100: 10 M rows 2.0 / 3.2-3.3
    // (the bf16 scan: fewer than 256 queries), 1 M rows 0.56-0.59 / 0.53
    // (k = 100 at 10 M rows was measured against the bf16 scan; the int8 batch scan, which such a search takes since, is at
    // 1.89 ms for 33 queries: the sweep stays with k <= 32)
    if (nq > 16) return k <= 32 && rows.n >= 50000 && rows.n < 4000000;
    return rows.n >= (k <= 32 ? 50000 : 1000000);
}

// one cascade stage of the int8 MFMA sweep (3..32 queries: k_sweep_mfma_i8); the int8 queries sit in ix->qh.p
int launch_sweep_mfma(css_index* ix, const Rows& rows, int nq, int64_t count, int64_t stride, int gm1, bool stage0,
                      hipStream_t st) {
    const int grid = (int)std::min<int64_t>((int64_t)ix->num_cus * 8, count);
    const signed char* q8 = reinterpret_cast<const signed char*>(ix->qh.p);
    const auto launch = [&](auto NG) -> int {   // fragment sets per lane
        return sweep_unrolled<12>(ix, stride == 1 && !stage0, [&](auto KS, auto MAIN) -> int {
            hipLaunchKernelGGL((k_sweep_mfma_i8<decltype(KS)::value, decltype(MAIN)::value, decltype(NG)::value>), dim3(grid),
                               dim3(256), 0, st, rows.x8, rows.x8s, q8, ix->qscale.p, ix->cthr.p, ix->cand_s.p, ix->cand_i.p,
                               ix->cand_n.p, rows.n, ix->dpad, nq, count, stride, gm1, stage0 ? 1 : 0, rows.mask);
            CSS_LAUNCH_CHECK();
            return CSS_OK;
        });
    };
    return nq <= 16 ? launch(IntC<1>()) : launch(IntC<2>());   // 17..32 queries: two fragment sets per lane
}

// one later stage of the int8 batch scan with the queries in registers (k_scan_qreg_i8): two 4-wave blocks per CU
inline int qreg_grid(const css_index* ix) { return std::max(8, ix->num_cus * 2 / 8 * 8); }
template <int KS>
int launch_scan_qreg_t(css_index* ix, const Rows& rows, int nqt, int64_t count, int64_t stride, int gm1,
                       bool main_stage, hipStream_t st) {
    const size_t lds = qr_lds_bytes<KS>();
    auto kern = main_stage ? k_scan_qreg_i8<KS, true> : k_scan_qreg_i8<KS, false>;
    int rc;
    if ((rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(qreg_grid(ix)), dim3(256), lds, st, (const unsigned char*)rows.x8,
                       reinterpret_cast<const signed char*>(ix->qh.p), (const float*)ix->cthr.p, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p,
                       rows.n, nqt, count, stride, gm1, rows.mask, (const float*)rows.x8s, (const float*)ix->qscale.p);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}
inline bool qreg_applies(const css_index* ix, int nqt) {
    return knn_env().qreg && (ix->dpad == 256 || ix->dpad == 512 || ix->dpad == 768) && (qreg_grid(ix) / 8) / nqt >= 1;
}
int launch_scan_qreg(css_index* ix, const Rows& rows, int nqt, int64_t count, int64_t stride, int gm1, bool main_stage,
                     hipStream_t st) {
    if (ix->dpad == 768) return launch_scan_qreg_t<12>(ix, rows, nqt, count, stride, gm1, main_stage, st);
    if (ix->dpad == 512) return launch_scan_qreg_t<8>(ix, rows, nqt, count, stride, gm1, main_stage, st);
    return launch_scan_qreg_t<4>(ix, rows, nqt, count, stride, gm1, main_stage, st);
}

// grid of the persistent k_scan_coarse launches and the largest query chunk it can serve: the nqt blocks
// that share a row tile must fit the grid / 8 blocks of one XCD group (a CPX partition has few CUs)
inline int coarse_grid(const css_index* ix) { return std::max(8, ix->num_cus / 8 * 8); }
inline int coarse_max_chunk(const css_index* ix) { return std::min(4096, coarse_grid(ix) / 8 * CZ_T); }

// ---- the candidate cascade of one chunk of queries (launch_scan_coarse).  Its rules -- kind, growth, schedule, error
// bound, tickets -- are css_knn_plan.h; here they meet the index: the workspace, the launch of a stage, the selects.
typedef void (*scan_fn)(const unsigned short*, const unsigned short*, const float*, float*, uint32_t*, int*, int64_t, int,
                        int, int64_t, int64_t, int, int*, const uint32_t*, const float*, const int*, const float*,
                        const float*);
constexpr int kPaceGroups = 512, kPaceStages = 20;   // sibling pacing counters of the batch scan (cpace)
struct CascadeCall {
    CascadeKind kind;
    bool i8;          // the scan reads the int8 rows ...
    bool i8q;         // ... with int8 queries (every kind but the VALU sweep, whose queries stay fp32)
    int q0, nq, k;    // queries [q0, q0 + nq) of ix->qpad.p; nq <= 4096
    int nq_pad, nqt;  // query rows the scan sees, and their tiles of CZ_T
    int l2;
    int growth;
    CascadePlan plan;
    bool fused;       // the VALU sweep's stages and the selects between them as ONE launch (k_sweep_cascade)
    FsSched tickets;  // ... its schedule
    // Second pass (batches on indexes whose rows can overflow a 4096-slot buffer at all): flagged queries -- band or
    // buffer overflow: dense clusters, duplicate floods -- are scanned once more, together, against the threshold the
    // exact scores of their buffered candidates give (k_coarse_select<true>), into CZ_CAP2-slot buffers; only what
    // overflows those too goes on to the exact fp32 sweep.  Round 2 sent every flagged query to that sweep (8 queries
    // per pass over the fp32 rows): 22 flagged of 1000 queries cost 2.9 ms of a 7 ms batch at 1 M clustered rows.
    // (the second pass reads the bf16 rows: a shadow-less range scanned from int8 scratch rows sends its flagged queries
    // straight to the exact sweep -- and, through the feedback of batch_uses_i8, the next searches to bf16 ranges)
    bool pass2;
    int f2;           // its query slots (a multiple of CZ_T)
    // one-eps thresholds from exactly scored top-k candidates (k_coarse_select): the int8 scan with int8 queries, whose
    // band is the widest (the scores are inner products: batch_uses_i8)
    bool exact_k;
    EpsSet eps, eps_p2;   // of the scan, and of the second pass (always bf16 rows and queries)
    scan_fn scan_stage0, scan_mid, scan_main;   // Batch: the kernel of stage 0, of a middle stage, of the main stage
    float* D;             // result rows of the chunk
    int64_t* I;
    // pointers into the index's buffers: null until cascade_workspace has grown them
    float *qpad, *qnorm2;
    int *gthr, *flags, *flag_list, *nflag;
    int *flag_listB, *nflagB;   // pass2: the queries left to the exact sweep
};

// the whole sweep cascade in one launch (k_sweep_cascade)
template <int NQ, int TT, bool I8>
int launch_sweep_cascade_t(css_index* ix, const Rows& rows, const CascadeCall& c, hipStream_t st) {
    const int steps = I8 ? (TT > 0 ? TT : (ix->dpad / 16 + 15) / 16) : 0;
    const size_t lds = (size_t)cz_fs_lds_floats(NQ, I8 ? 256 * steps : ix->dpad) * sizeof(float);
    auto kern = k_sweep_cascade<NQ, TT, I8>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    // as many blocks as the chip holds at once (a wave leaves only when the tickets run out: more blocks would start at
    // the very end, load the queries and find nothing to do); nothing depends on the blocks being co-resident, and no
    // result on the grid: tickets are drawn from a counter
    int& per_cu_cached = ix->fs_occ[(const void*)kern];   // (asked once per index -- one device, one row width -- and kernel; caller holds ws_mu)
    if (per_cu_cached == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_cached, kern, 256, lds) != hipSuccess || per_cu_cached < 1))
        per_cu_cached = 1;
    const int per_cu = std::min(per_cu_cached, 3);   // (12 waves per CU already draw the whole HBM rate: 2 / 3 / 4 blocks 1.305 / 1.302 / 1.316 ms at 10 M rows)
    const FsSched& sc = c.tickets;
    const int grid = (int)std::min<int64_t>((int64_t)ix->num_cus * std::min(per_cu, 8), (sc.first[sc.nstage] + 3) / 4);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, I8 ? (const void*)rows.x8 : (const void*)rows.xh,
                       I8 ? (const float*)rows.x8s : (const float*)nullptr, (const float*)c.qpad, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p, ix->cthr.p,
                       c.flags, rows.n, ix->dpad, c.nq, sc, ix->fs_state.p, rows.mask,
                       ix->metric == CSS_METRIC_L2 ? rows.xnorm2 : nullptr, (const float*)c.qnorm2, (const int*)ix->maxn2.p, c.eps.eps_rel, c.l2, c.k,
                       c.eps.measured, knn_env().fs_spins);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// What one chunk's cascade is, decided once.  use_i8: which shadow rows this SEARCH reads (the caller's decision: the
// per-index feedback is consulted once per search, not per chunk).
CascadeCall cascade_call(const css_index* ix, const Rows& rows, CascadeKind kind, bool use_i8, int q0, int nq, int k,
                         float* D_dev, int64_t* I_dev) {
    const KnnEnv& env = knn_env();
    const bool batch = kind == CascadeKind::Batch;
    CascadeCall c{};
    c.kind = kind;
    c.i8 = use_i8;
    c.i8q = use_i8 && kind != CascadeKind::SweepValu;
    c.q0 = q0, c.nq = nq, c.k = k;
    // (the int8 MFMA sweep: 16 or 32 int8 query rows, zero padded)
    c.nq_pad = batch ? (nq + CZ_T - 1) / CZ_T * CZ_T : (kind == CascadeKind::SweepMfma ? (nq <= 16 ? 16 : 32) : nq);
    c.nqt = batch ? c.nq_pad / CZ_T : 1;
    c.l2 = ix->metric == CSS_METRIC_L2 ? 1 : 0;
    c.growth = cascade_growth(kind, use_i8, k, rows.n, env.growth, env.growth_sweep);
    c.plan = cascade_plan((rows.n + CZ_T - 1) / CZ_T, c.growth, cascade_fills_stage0(kind), cascade_splits_last(kind, use_i8));
    // 1..4 queries: one launch, quarter tiles as tickets in stage order (measured, ms one launch / one per stage: 10 M rows,
    // 1 query k = 10 1.35 / 1.41, k = 100 1.40 / 1.56, 2 queries 1.40 / 1.47, 4 queries 2.68 / 2.69; 100 k rows: 0.085 /
    // 0.095, 0.118 / 0.125, but 2 queries 0.117 / 0.111, 4: 0.186 / 0.155) -- where the tickets can state the plan
    c.fused = kind == CascadeKind::SweepValu && env.sweep_fused && (env.sweep_fused == 2 || nq == 1 || rows.n >= 1000000) &&
              cascade_tickets(c.plan, c.growth, c.tickets.first, c.tickets.stride, c.tickets.gm1);
    if (c.fused) c.tickets.nstage = c.plan.n;
    c.pass2 = batch && ix->dpad % 128 == 0 && rows.n > CZ_CAP && rows.xh != nullptr;
    c.f2 = c.pass2 ? std::min(c.nq_pad, kF2Max) : 0;
    c.exact_k = c.i8q && k * 2 <= CZ_EXK;
    // measured = the word of maxn2 that holds the rows' error: 1 = bf16 rows, 2 = int8 rows
    c.eps = EpsSet{cascade_eps_rel(kind, use_i8, ix->dpad), nullptr, use_i8 ? 2 : 1};
    c.eps_p2 = EpsSet{cascade_eps_rel(CascadeKind::Batch, false, ix->dpad), nullptr, 1};
    if (batch) {
        // the 8-phase ping-pong loop (k_scan_coarse8) wherever its shape constraints hold (batch_uses_i8 implies it)
        const bool loop8 = ix->dpad % 128 == 0;
        const bool i8b = use_i8;
        c.scan_stage0 = i8b ? k_scan_coarse8<true, false, CZ_CAP, true>
                            : (loop8 ? k_scan_coarse8<true, false> : k_scan_coarse<true, false>);
        c.scan_mid = i8b ? k_scan_coarse8<false, false, CZ_CAP, true>
                         : (loop8 ? k_scan_coarse8<false, false> : k_scan_coarse<false, false>);
        c.scan_main = i8b ? k_scan_coarse8<false, true, CZ_CAP, true>
                          : (loop8 ? k_scan_coarse8<false, true> : k_scan_coarse<false, true>);
    }
    c.D = D_dev + (size_t)q0 * k;
    c.I = I_dev + (size_t)q0 * k;
    return c;
}

// Every growth of the chunk's buffers, and only then the pointers into them.  A DevBuf that grows frees its old memory,
// so NO pointer into one of these buffers is formed above the last growth: the steps of the cascade take theirs from the
// call, which gets them at the end of this function, or from the index after it has run.  (Until round 4 the int8 queries'
// error norms grew below the point where their pointer was taken, so the selects of the first int8 search with more
// queries than any before read the freed, shorter buffer: zeros on a fresh device, i.e. a band without the query term;
// stale bytes otherwise, i.e. everything flagged -- 744 of 1000 queries and 33 ms in the third index of one process,
// tools/seq_probe.py.)
int cascade_workspace(css_index* ix, CascadeCall& c, hipStream_t st) {
    const size_t nq_pad = (size_t)c.nq_pad;
    int rc;
    // rounded query rows: bf16, or int8 (into the same buffer: half its bytes) with their scales and error norms
    if (c.kind != CascadeKind::SweepValu && (rc = ix->qh.grow(nq_pad * ix->dpad)) != CSS_OK) return rc;
    if (c.i8q && (rc = ix->qscale.grow(nq_pad)) != CSS_OK) return rc;
    if (c.i8q && (rc = ix->qerr2_i8.grow((size_t)c.q0 + nq_pad)) != CSS_OK) return rc;
    if ((rc = grow_candidate_ws(ix, nq_pad, c.k)) != CSS_OK) return rc;
    if (c.pass2) {
        const size_t qh2_before = ix->qh2.cap;
        if ((rc = ix->qh2.grow((size_t)c.f2 * ix->dpad)) != CSS_OK) return rc;
        // slots beyond the flagged count are scanned with a +inf threshold; their rows must still be finite numbers
        if (ix->qh2.cap != qh2_before) CSS_HIP_TRY(hipMemsetAsync(ix->qh2.p, 0, ix->qh2.cap * sizeof(unsigned short), st));
        if ((rc = ix->thr2.grow((size_t)c.f2)) != CSS_OK) return rc;
        if ((rc = ix->cand_n2.grow((size_t)c.f2 * CZ_NS)) != CSS_OK) return rc;
        if ((rc = ix->cand_s2.grow((size_t)c.f2 * CZ_CAP2)) != CSS_OK) return rc;
        if ((rc = ix->cand_i2.grow((size_t)c.f2 * CZ_CAP2)) != CSS_OK) return rc;
        if ((rc = ix->flagB.grow(nq_pad + 2)) != CSS_OK) return rc;
    }
    if (c.fused && (rc = ix->fs_state.grow((size_t)CZ_FS_WORDS)) != CSS_OK) return rc;
    if (c.kind == CascadeKind::Batch && (rc = ix->cpace.grow((size_t)kPaceGroups * kPaceStages)) != CSS_OK) return rc;
    // ---- the last growth is above this line
    c.qpad = ix->qpad.p + (size_t)c.q0 * ix->dpad;
    c.qnorm2 = ix->qnorm2.p + c.q0;
    c.gthr = ix->gthr.p + c.q0;
    c.flags = ix->cflags.p;
    c.flag_list = ix->cflags.p + nq_pad;
    c.nflag = ix->cflags.p + 2 * nq_pad;
    if (c.pass2) {
        c.flag_listB = ix->flagB.p;
        c.nflagB = ix->flagB.p + nq_pad;
    }
    // the queries' own rounding error (cz_eps): none for the fp32 queries of the VALU sweep
    if (c.kind != CascadeKind::SweepValu) c.eps.qerr2 = c.i8q ? ix->qerr2_i8.p + c.q0 : ix->qerr2.p + c.q0;
    c.eps_p2.qerr2 = ix->qerr2.p + c.q0;
    return CSS_OK;
}

// int8 query rows, their scales and error norms
int launch_queries_to_i8(css_index* ix, const CascadeCall& c, hipStream_t st) {
    hipLaunchKernelGGL(k_rows_to_i8, dim3((unsigned)((c.nq_pad + 3) / 4)), dim3(256), 0, st, (const float*)c.qpad,
                       reinterpret_cast<signed char*>(ix->qh.p), ix->qscale.p, ix->qerr2_i8.p + c.q0, c.nq, c.nq_pad, ix->dpad);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Thresholds, counters and flags of the chunk cleared in one launch (k_coarse_init), the rounded query rows around it.
// q_raw != null (sweeps only): the raw query rows, still to be prepared (normalize_q as in search_dev_enqueue) -- the
// init launch does it, so the int8 queries of the MFMA sweep are made behind it; a batch's queries come prepared.
int cascade_init(css_index* ix, const CascadeCall& c, const float* q_raw, int normalize_q, hipStream_t st) {
    const bool batch = c.kind == CascadeKind::Batch;
    int rc;
    if (batch && c.i8) {
        if ((rc = launch_queries_to_i8(ix, c, st)) != CSS_OK) return rc;
    } else if (batch) {
        const int64_t ne = (int64_t)c.nq_pad * ix->dpad;
        hipLaunchKernelGGL(k_rows_to_bf16, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, (const float*)c.qpad, ix->qh.p,
                           (int64_t)c.nq, (int64_t)c.nq_pad, ix->dpad);
        CSS_LAUNCH_CHECK();
    }
    const int npace = batch ? kPaceGroups * kPaceStages : 0;
    const int ninit = std::max(std::max(std::max(std::max(c.nq_pad, npace), c.f2), c.fused ? CZ_FS_KEYWORDS : 0),
                               q_raw != nullptr ? c.nq * 64 : 0);   // (query prep: one wave per query)
    hipLaunchKernelGGL(k_coarse_init, dim3((ninit + 255) / 256), dim3(256), 0, st, ix->cthr.p, ix->cand_n.p, c.flags,
                       c.nflag, c.nq, c.nq_pad, (int)(c.plan.st[0].count * CZ_T), batch ? ix->cpace.p : (int*)nullptr, npace,
                       c.pass2 ? ix->cand_n2.p : (int*)nullptr, c.pass2 ? ix->thr2.p : (float*)nullptr, c.nflagB, c.f2,
                       c.fused ? ix->fs_state.p : (int*)nullptr, q_raw, c.qpad, c.qnorm2, ix->qerr2.p + c.q0, ix->dim, ix->dpad,
                       normalize_q);
    CSS_LAUNCH_CHECK();
    return c.kind == CascadeKind::SweepMfma ? launch_queries_to_i8(ix, c, st) : CSS_OK;
}

// the VALU sweep: all stages in one launch, or stage by stage
int launch_sweep_cascade(css_index* ix, const Rows& rows, const CascadeCall& c, hipStream_t st) {
    return sweep_nq_slots(c.nq, [&](auto NQ) -> int {
        if (c.i8)
            return sweep_unrolled<3>(ix, false, [&](auto TT, auto) -> int {
                return launch_sweep_cascade_t<decltype(NQ)::value, decltype(TT)::value, true>(ix, rows, c, st);
            });
        return sweep_unrolled<6>(ix, false, [&](auto TT, auto) -> int {
            return launch_sweep_cascade_t<decltype(NQ)::value, decltype(TT)::value, false>(ix, rows, c, st);
        });
    });
}
int launch_sweep_coarse(css_index* ix, const Rows& rows, const CascadeCall& c, int64_t count, int64_t stride, int gm1,
                        bool stage0, hipStream_t st) {
    return sweep_nq_slots(c.nq, [&](auto NQ) -> int {
        if (c.i8)
            return sweep_unrolled<3>(ix, stride == 1 && !stage0, [&](auto TT, auto MAIN) -> int {
                return launch_sweep_coarse_i8_t<decltype(NQ)::value, decltype(TT)::value, decltype(MAIN)::value>(
                    ix, rows, c.qpad, c.nq, count, stride, gm1, stage0, st);
            });
        return sweep_unrolled<6>(ix, stride == 1 && !stage0, [&](auto TT, auto MAIN) -> int {
            return launch_sweep_coarse_t<decltype(NQ)::value, decltype(TT)::value, decltype(MAIN)::value>(
                ix, rows, c.qpad, c.nq, count, stride, gm1, stage0, st);
        });
    });
}

// stage si of the plan on the kernel of the call's kind
int cascade_stage(css_index* ix, const Rows& rows, const CascadeCall& c, int si, hipStream_t st) {
    const CascadeStage& s = c.plan.st[si];
    if (s.count <= 0) return CSS_OK;
    const bool stage0 = si == 0, main_stage = s.stride == 1 && !stage0;
    const int gm1 = cascade_gm1(c.plan, c.growth, si);
    if (c.kind == CascadeKind::SweepMfma) {
        ProfScope ps(main_stage ? "knn_sweep_mfma_main" : "knn_sweep_mfma_stage", st);
        return launch_sweep_mfma(ix, rows, c.nq, s.count, s.stride, gm1, stage0, st);
    }
    if (c.kind == CascadeKind::SweepValu) {
        ProfScope ps(main_stage ? "knn_sweep_coarse_main" : "knn_sweep_coarse_stage", st);
        return launch_sweep_coarse(ix, rows, c, s.count, s.stride, gm1, stage0, st);
    }
    ProfScope ps(main_stage ? "knn_scan_coarse_main" : "knn_scan_coarse_stage", st);
    // int8 rows, later stages: the queries stay in registers (k_scan_qreg_i8) -- from two (row tile, query tile) pairs
    // per block on: a block first loads its 256 queries.  ms per search, k = 10, 64 / 256 / 1000 queries, minimum
    // 0 / 1024 / 4096 / never: 300 k rows 0.31, 0.35, 0.56 / 0.26, 0.31, 0.53 / 0.26, 0.31, 0.56 / 0.25, 0.31, 0.56;
    // 3 M rows (1024 / 4096 / never) 0.70, 0.79, 2.25 / 0.73, 0.84, 2.28 / 0.78, 0.90, 2.56; 10 M rows 1.88, 1.99,
    // 6.45 / 1.88, 2.01, 6.52 / 2.05, 2.27, 7.36.
    if (c.i8 && !stage0 && qreg_applies(ix, c.nqt) && s.count * c.nqt >= knn_env().qreg_min)
        return launch_scan_qreg(ix, rows, c.nqt, s.count, s.stride, gm1, main_stage, st);
    // (int8 rows: no sibling pacing -- a row tile fetched by every query-tile block on its own is still only
    // ~3.5 TB/s worst case at this scan's speed, and the coupling costs more than the HBM traffic it saves:
    // 9.65 vs 9.02 ms per batch; the bf16 scan reads twice the bytes per row and needs it)
    const int grid = coarse_grid(ix);
    int* pace = (!c.i8 && grid / 8 <= kPaceGroups / 8 && si < kPaceStages) ? ix->cpace.p + (size_t)si * kPaceGroups : nullptr;
    hipLaunchKernelGGL(stage0 ? c.scan_stage0 : (main_stage ? c.scan_main : c.scan_mid), dim3(grid), dim3(512),
                       (size_t)CZ_NST * CZ_STAGE, st, c.i8 ? reinterpret_cast<const unsigned short*>(rows.x8) : rows.xh, ix->qh.p,
                       ix->cthr.p, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p, rows.n, ix->dpad, c.nqt, s.count, s.stride, gm1, pace,
                       rows.mask, c.l2 ? rows.xnorm2 : nullptr,   // L2: coarse score = 2 x.q - ||x||^2
                       (const int*)nullptr, c.i8 ? rows.x8s : nullptr, c.i8 ? ix->qscale.p : nullptr);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// the select between two stages (the next threshold), and the one behind the last: band, exact rescoring, results
int cascade_select(css_index* ix, const Rows& rows, const CascadeCall& c, bool final, hipStream_t st) {
    if (final)
        return launch_final_select(ix, rows, c.nq, c.k, c.eps, c.eps_p2, c.exact_k, c.l2, 0, c.qpad, c.qnorm2, c.gthr, c.flags,
                                   c.nflag, c.flag_list, c.D, c.I, c.pass2 ? ix->thr2.p : nullptr,
                                   c.pass2 ? ix->qh2.p : nullptr, c.f2, st);
    hipLaunchKernelGGL(k_coarse_select<false>, dim3(c.nq), dim3(256), 0, st, ix->cand_s.p, ix->cand_i.p, ix->cand_n.p,
                       ix->cthr.p, c.flags, c.nflag, c.flag_list, (const float*)c.qnorm2, ix->maxn2.p, c.eps.eps_rel, c.l2, c.k, 0, c.gthr,
                       c.eps.qerr2, c.eps.measured, ix->fix_s.p, ix->fix_i.p, ix->fix_lock.p,
                       c.exact_k ? (const float*)c.qpad : (const float*)nullptr,
                       c.exact_k ? (const float*)rows.xb : (const float*)nullptr, ix->dpad);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// the second pass over the flagged queries of a batch (CascadeCall::pass2); every launch reads the flagged count from
// device memory and returns at once when there is nothing to do
int cascade_pass2(css_index* ix, const Rows& rows, const CascadeCall& c, hipStream_t st) {
    ProfScope ps("knn_coarse_pass2", st);
    const size_t lds = (size_t)CZ_NST * CZ_STAGE;
    const scan_fn f_all = k_scan_coarse8<false, true, CZ_CAP2>;   // every row tile against thr2 (the gate also makes tile = ordinal)
    int rc;
    if ((rc = css::ensure_dynamic_lds((const void*)f_all, lds, ix->device)) != CSS_OK) return rc;
    const int grid = coarse_grid(ix);
    const int stage_idx = c.plan.n;   // (its pacing counters: behind the stages')
    int* pace = (grid / 8 <= kPaceGroups / 8 && stage_idx < kPaceStages) ? ix->cpace.p + (size_t)stage_idx * kPaceGroups : nullptr;
    hipLaunchKernelGGL(f_all, dim3(grid), dim3(512), lds, st, rows.xh, ix->qh2.p, ix->thr2.p, ix->cand_s2.p, ix->cand_i2.p,
                       ix->cand_n2.p, rows.n, ix->dpad, c.f2 / CZ_T, c.plan.ntiles, (int64_t)1, 1 << 30, pace, rows.mask,
                       c.l2 ? rows.xnorm2 : nullptr, (const int*)c.nflag, (const float*)nullptr, (const float*)nullptr);
    hipLaunchKernelGGL(k_rescore_parts<true>, dim3(kRescoreGrid), dim3(256), 0, st, ix->cand_s2.p, ix->cand_i2.p, ix->cand_n2.p,
                       CZ_CAP2, c.f2, c.nflag, c.flag_list, ix->thr2.p, c.l2, (const float*)c.qpad, rows.xb, ix->dpad, (const int*)nullptr,
                       (const int*)nullptr);
    hipLaunchKernelGGL(k_coarse_select2<CZ_CAP2>, dim3(c.f2), dim3(256), 0, st, ix->cand_s2.p, ix->cand_i2.p, ix->cand_n2.p, c.nflag,
                       c.flag_list, c.f2, c.nflagB, c.flag_listB, c.l2, c.k, rows.id_base, c.D, c.I);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Coarse scan + exact rescoring (css_knn_coarse.h) for queries [q0, q0 + nq) of ix->qpad.p; nq <= 4096.
// Everything is enqueued on `st`; nothing waits for the device (flagged queries are fixed up on the device).
// kind, use_i8: decided once per search by the caller (search_dev_enqueue / search_noshadow_ranges); record_fb: this is
// the search's last chunk, whose flagged count is what the int8 feedback sees.  q_raw, normalize_q: cascade_init.
int launch_scan_coarse(css_index* ix, const Rows& rows, int q0, int nq, int k, float* D_dev, int64_t* I_dev, hipStream_t st,
                       const SweepGeom& sg, CascadeKind kind, bool use_i8, bool record_fb, const float* q_raw = nullptr,
                       int normalize_q = 0) {
    const bool batch = kind == CascadeKind::Batch;
    CascadeCall c = cascade_call(ix, rows, kind, use_i8, q0, nq, k, D_dev, I_dev);
    int rc;
    if ((rc = cascade_workspace(ix, c, st)) != CSS_OK) return rc;
    ix->last_nflag = c.nflag;
    ix->last_nswept = c.pass2 ? c.nflagB : c.nflag;
    if ((rc = cascade_init(ix, c, q_raw, normalize_q, st)) != CSS_OK) return rc;
    if (batch)
        for (scan_fn f : {c.scan_stage0, c.scan_mid, c.scan_main})
            if ((rc = css::ensure_dynamic_lds((const void*)f, (size_t)CZ_NST * CZ_STAGE, ix->device)) != CSS_OK) return rc;
    CSS_REQUIRE(!batch || (coarse_grid(ix) / 8) / c.nqt >= 1, "css_index_search: %d query tiles do not fit a grid of %d blocks",
                c.nqt, coarse_grid(ix));
    {
        ProfScope all(batch ? "knn_coarse_cascade" : "knn_sweep_cascade", st);
        if (c.fused) {
            {
                ProfScope ps("knn_sweep_fused", st);
                if ((rc = launch_sweep_cascade(ix, rows, c, st)) != CSS_OK) return rc;
            }
            if ((rc = cascade_select(ix, rows, c, true, st)) != CSS_OK) return rc;
        } else {
            for (int si = 0; si < c.plan.n; ++si) {
                if ((rc = cascade_stage(ix, rows, c, si, st)) != CSS_OK) return rc;
                if ((rc = cascade_select(ix, rows, c, si == c.plan.n - 1, st)) != CSS_OK) return rc;
            }
        }
    }
    // feedback for batch_i8_wanted / sweep_uses_i8: the last chunk of a search speaks for it
    if (record_fb && use_i8 && batch && knn_env().batch_i8 == 1 && (rc = i8_feedback_record(ix->fb_batch, c.nflag, nq, st)) != CSS_OK) return rc;
    if (record_fb && use_i8 && !batch && (rc = i8_feedback_record(ix->fb_sweep, c.nflag, nq, st)) != CSS_OK) return rc;
    if (c.pass2 && (rc = cascade_pass2(ix, rows, c, st)) != CSS_OK) return rc;
    // queries whose candidate buffer or band overflowed (thousands of duplicate rows, a zero query) -- and, behind a second
    // pass, its buffers too (tens of thousands of rows inside one band): exact fp32 sweep on the device, two launches that
    // return at once when the flag count is zero
    return launch_fixup(ix, rows, c.qpad, nq, k, c.gthr, c.pass2 ? c.flag_listB : c.flag_list, c.pass2 ? c.nflagB : c.nflag, c.D,
                        c.I, sg, st);
}

// grid of the exact fp32 sweeps (k_scan_small, k_range_small, k_scan_prior, k_scan_examples, k_facet_small) over the rows in view:
// enough blocks to fill the chip (8 per CU) but at least ~64 row groups of work each
void sweep_grid(const css_index* ix, const Rows& rows, int* G, int64_t* gpb) {
    const int64_t ngroups = (rows.n + 3) / 4;
    const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>((int64_t)ix->num_cus * 8, (ngroups + 63) / 64));
    *gpb = (ngroups + G0 - 1) / G0;
    *G = (int)((ngroups + *gpb - 1) / *gpb);
}

// sweep geometry of the small-batch kernel (also the exact fix-up of the candidate paths) for the rows in view
int make_sweep_geom(const css_index* ix, const Rows& rows, int k, SweepGeom* sg) {
    sg->nq_sweep = (int)std::min<int64_t>(16, (64 * 1024) / ((int64_t)ix->dpad * 4 + (int64_t)k * 8 + 8));
    CSS_REQUIRE(sg->nq_sweep >= 1, "css_index_search: dim=%d too large for the scan kernel", ix->dim);
    sweep_grid(ix, rows, &sg->G, &sg->gpb);
    return CSS_OK;
}

// ------------------------------------------------------------------ range search (css_knn_range.h)
#include "css_knn_range.h"

constexpr int kRangeSlots = css_index::kRangeSlots;
constexpr size_t kRangeInitialCap = 4096;    // pool entries per slot before the first growth

template <int NQ, int TT, int METRIC>
int launch_range_small_t(css_index* ix, const Rows& rows, const float* qpad, int nq_real, float radius, int G,
                         int64_t gpb, hipStream_t st) {
    const size_t lds = (size_t)NQ * ix->dpad * 4;
    auto kern = k_range_small<NQ, TT, METRIC>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    ProfScope ps("knn_range_small", st);
    hipLaunchKernelGGL(kern, dim3(G), dim3(256), lds, st, (const float4*)rows.xb, qpad, rows.n, ix->dpad / 64, gpb, nq_real,
                       rows.mask, radius, ix->range_cnt.p, ix->range_s.p, ix->range_i.p, (unsigned int)ix->range_cap());
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int NQ>
int launch_range_small_nq(css_index* ix, const Rows& rows, const float* qpad, int nq_real, float radius, int G,
                          int64_t gpb, hipStream_t st) {
    return sweep_variant(ix, [&](auto TT, auto M) {
        return launch_range_small_t<NQ, decltype(TT)::value, decltype(M)::value>(ix, rows, qpad, nq_real, radius, G, gpb, st);
    });
}

// queries per sweep: the largest instantiated NQ (16, 8, 2) whose query rows fit 64 KiB of LDS (dim <= 8192: at least 2)
int range_nq_sweep(const css_index* ix) {
    const int64_t fit = (64 * 1024) / ((int64_t)ix->dpad * 4);
    return fit >= 16 ? 16 : (fit >= 8 ? 8 : 2);
}

// One sweep of all rows for queries qpad[0 .. nqc) (nqc <= range_nq_sweep): counters zeroed, kernel, counters back on
// the host (waits for the stream).
int range_sweep(css_index* ix, const Rows& rows, const float* qpad, int nqc, float radius, unsigned int* cnt_host,
                hipStream_t st) {
    int G;
    int64_t gpb;
    sweep_grid(ix, rows, &G, &gpb);
    CSS_HIP_TRY(hipMemsetAsync(ix->range_cnt.p, 0, kRangeSlots * sizeof(unsigned int), st));
    const int rc = sweep_slots(nqc, [&](auto NQ) {
        return launch_range_small_nq<decltype(NQ)::value>(ix, rows, qpad, nqc, radius, G, gpb, st);
    });
    if (rc != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(cnt_host, ix->range_cnt.p, kRangeSlots * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

// The hit pool with `cap` entries per slot (nothing of the old one is kept: a grown pool is filled by a new sweep).
// No room: CSS_ERR_OOM, the pool is gone (the next call starts from the initial size) and the index is untouched.
int range_pool_alloc(css_index* ix, size_t cap) {
    return try_exact_pair(ix->range_s, ix->range_i, kRangeSlots * cap) ? CSS_OK : CSS_ERR_OOM;
}

// ------------------------------------------------------------------ facet counts (css_knn_facets.h)
#include "css_knn_facets.h"

constexpr int64_t kFacetMaxEntries = (int64_t)CSS_MAX_FACET_BUCKETS;   // table entries of one sweep
constexpr size_t kFacetEntryBytes = sizeof(unsigned long long) + sizeof(unsigned int);   // key + count
constexpr size_t kLdsPerCu = 160 * 1024;      // gfx950

// Does the [nqc][nbuckets] table of a sweep go to LDS?  The library's rule is a number of blocks that must still fit
// one CU (160 KB) with the NQ query rows and the table each: ONE block for NQ <= 2, TWO for NQ = 8 / 16.  Measured at
// 10 M x 768 (profiles/facets_10M.json): the one- and two-query sweeps are HBM bound and the LDS table
// never lost to the global one, down to a single block per CU; the 8- and 16-query sweeps are VALU / LDS bound: with
// rare hits the LDS table costs up to 3 % (8 queries) and 9 % (16 queries) while two blocks fit and 37-51 % at one, and
// with half the rows hitting it wins 2x to 11x at two blocks or more and barely at one.  (Keeping k_range_small's own occupancy, three to four blocks, was the first rule: it sent 16 queries x 64
// buckets to global memory, 2.2x slower with half the rows hitting.)  css_index_set_facet_lds_entries replaces the rule
// by a fixed entry count (0: never), still inside the 160 KB one block can have.
bool facet_lds_fits(const css_index* ix, int NQ, int64_t entries) {
    const size_t qbytes = (size_t)NQ * ix->dpad * 4, tbytes = (size_t)entries * kFacetEntryBytes;
    if (qbytes + tbytes > kLdsPerCu) return false;
    if (ix->facet_lds_entries >= 0) return entries <= ix->facet_lds_entries;
    return qbytes + tbytes <= kLdsPerCu / (NQ <= 2 ? 1 : 2);
}

template <int NQ, int TT, int METRIC, bool LDS_TABLE>
int launch_facet_small_t(css_index* ix, const Rows& rows, const float* qpad, int nq_real, float radius, const int32_t* bucket,
                         int nbuckets, int G, int64_t gpb, hipStream_t st) {
    const size_t E = (size_t)nq_real * nbuckets;
    const size_t lds = (size_t)NQ * ix->dpad * 4 + (LDS_TABLE ? E * kFacetEntryBytes : 0);
    auto kern = k_facet_small<NQ, TT, METRIC, LDS_TABLE>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    unsigned int* words = reinterpret_cast<unsigned int*>(ix->facet_tab.p + E);   // [16 | 16 | E counts]
    ProfScope ps("knn_facet_small", st);
    hipLaunchKernelGGL(kern, dim3(G), dim3(256), lds, st, (const float4*)rows.xb, qpad, rows.n, ix->dpad / 64, gpb, nq_real,
                       rows.mask, radius, bucket, nbuckets, words, words + 32, ix->facet_tab.p);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int NQ>
int launch_facet_small_nq(css_index* ix, const Rows& rows, const float* qpad, int nq_real, float radius, const int32_t* bucket,
                          int nbuckets, bool lds_table, int G, int64_t gpb, hipStream_t st) {
    return sweep_variant(ix, [&](auto TT, auto M) {
        return lds_table ? launch_facet_small_t<NQ, decltype(TT)::value, decltype(M)::value, true>(ix, rows, qpad, nq_real, radius, bucket, nbuckets, G, gpb, st)
                         : launch_facet_small_t<NQ, decltype(TT)::value, decltype(M)::value, false>(ix, rows, qpad, nq_real, radius, bucket, nbuckets, G, gpb, st);
    });
}

// 8-byte words of the table of a sweep with E entries: [E keys | 32 + E uint32]
inline size_t facet_tab_words(size_t E) { return E + (32 + E + 1) / 2; }

// One sweep of all rows for queries qpad[0 .. nqc): table zeroed, kernel, table back in `tab_host` (waits for the
// stream).  *lds: the placement that ran.
int facet_sweep(css_index* ix, const Rows& rows, const float* qpad, int nqc, float radius, const int32_t* bucket, int nbuckets,
                unsigned long long* tab_host, bool* lds, hipStream_t st) {
    int G;
    int64_t gpb;
    sweep_grid(ix, rows, &G, &gpb);
    const size_t words = facet_tab_words((size_t)nqc * nbuckets);
    CSS_HIP_TRY(hipMemsetAsync(ix->facet_tab.p, 0, words * sizeof(unsigned long long), st));
    const int rc = sweep_slots(nqc, [&](auto NQ) {
        *lds = facet_lds_fits(ix, decltype(NQ)::value, (int64_t)nqc * nbuckets);
        return launch_facet_small_nq<decltype(NQ)::value>(ix, rows, qpad, nqc, radius, bucket, nbuckets, *lds, G, gpb, st);
    });
    if (rc != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(tab_host, ix->facet_tab.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    return CSS_OK;
}

// ------------------------------------------------------------------ prior-weighted search (css_knn_prior.h)
#include "css_knn_prior.h"
#include "css_lexical.h"
#include "css_sparse.h"
#include "css_token_codec.h"
#include "css_tokens.h"
#include "css_tokens_batch.h"
#include "css_tokens_lists.h"
#include "css_token_prune.h"
#include "css_where.h"
#include "css_sigterms.h"

// HASP: the index has a prior column (false: every prior is 0, the kernel loads none)
template <int NQ, int TT, int METRIC, bool HASP>
int launch_scan_prior_p(css_index* ix, const Rows& rows, const float* qpad, int nq_real, int k, float weight, int* gthr,
                        const SweepGeom& sg, hipStream_t st) {
    const size_t lds = (size_t)NQ * ix->dpad * 4 + (size_t)NQ * k * 8 + NQ * 8;   // (k_scan_small's, plain sweep)
    auto kern = k_scan_prior<NQ, TT, METRIC, HASP>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    ProfScope ps("knn_scan_prior", st);
    hipLaunchKernelGGL(kern, dim3(sg.G), dim3(256), lds, st, (const float4*)rows.xb, qpad, rows.n, ix->dpad / 64, k, sg.gpb,
                       gthr, ix->part_s.p, ix->part_i.p, nq_real, rows.mask, rows.priors, weight);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int NQ, int TT, int METRIC>
int launch_scan_prior_t(css_index* ix, const Rows& rows, const float* qpad, int nq_real, int k, float weight, int* gthr,
                        const SweepGeom& sg, hipStream_t st) {
    return rows.priors ? launch_scan_prior_p<NQ, TT, METRIC, true>(ix, rows, qpad, nq_real, k, weight, gthr, sg, st)
                       : launch_scan_prior_p<NQ, TT, METRIC, false>(ix, rows, qpad, nq_real, k, weight, gthr, sg, st);
}

template <int NQ>
int launch_scan_prior_nq(css_index* ix, const Rows& rows, const float* qpad, int nq_real, int k, float weight, int* gthr,
                         const SweepGeom& sg, hipStream_t st) {
    return sweep_variant(ix, [&](auto TT, auto M) {
        return launch_scan_prior_t<NQ, decltype(TT)::value, decltype(M)::value>(ix, rows, qpad, nq_real, k, weight, gthr, sg, st);
    });
}

// search_chunk_small with the prior sweep: queries [q0, q0+nqc) (nqc <= sg.nq_sweep) against the rows, fused values
// and ids to D/I rows q0...
int search_chunk_prior(css_index* ix, const Rows& rows, int q0, int nqc, int k, float weight, const SweepGeom& sg,
                       float* D_dev, int64_t* I_dev, hipStream_t st) {
    int* gthr = ix->gthr.p + q0;
    hipLaunchKernelGGL(k_fill_int, dim3(1), dim3(64), 0, st, gthr, nqc, host_f2key(-INFINITY));
    CSS_LAUNCH_CHECK();
    const float* qp = ix->qpad.p + (size_t)q0 * ix->dpad;
    const int rc = sweep_slots(nqc, [&](auto NQ) {
        return launch_scan_prior_nq<decltype(NQ)::value>(ix, rows, qp, nqc, k, weight, gthr, sg, st);
    });
    return rc != CSS_OK ? rc : launch_merge_final(ix, rows, q0, nqc, k, sg, D_dev, I_dev, st);
}

// ------------------------------------------------------------------ k-means step (css_kmeans.h)
#include "css_kmeans.h"
// ------------------------------------------------------------------ Gram matrix and linear transform (css_pca.h)
#include "css_pca.h"

// ------------------------------------------------------------------ search by examples (css_knn_examples.h)
#include "css_knn_examples.h"

// the sweep's dynamic LDS: the example table, ONE list of k keys and rows, the lock pair, the excluded rows
inline size_t examples_lds(int nq_slots, int dpad, int k) {
    return (size_t)nq_slots * dpad * 4 + (size_t)k * 8 + 8 + kMaxExamples * 4;
}
// NQ of the sweep for m examples
inline int examples_slots(int m) {
    return sweep_slots(m, [](auto NQ) { return (int)decltype(NQ)::value; });
}

struct ExampleArgs {
    int npos, m;              // positives, all examples (the table is [m][dpad], positives first)
    float gamma;
    const uint32_t* excl;     // local rows never returned
    int nexcl;
};

template <int NQ, int TT, int METRIC>
int launch_scan_examples_t(css_index* ix, const Rows& rows, const float* epad, int k, const ExampleArgs& ea, int* gthr,
                           const SweepGeom& sg, hipStream_t st) {
    const size_t lds = examples_lds(NQ, ix->dpad, k);
    auto kern = k_scan_examples<NQ, TT, METRIC>;
    int rc;
    if (lds > 48 * 1024 && (rc = css::ensure_dynamic_lds((const void*)kern, lds, ix->device)) != CSS_OK) return rc;
    ProfScope ps("knn_scan_examples", st);
    hipLaunchKernelGGL(kern, dim3(sg.G), dim3(256), lds, st, (const float4*)rows.xb, epad, rows.n, ix->dpad / 64, k, sg.gpb,
                       gthr, ix->part_s.p, ix->part_i.p, ea.npos, ea.m, ea.gamma, rows.mask, ea.excl, ea.nexcl);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

template <int NQ>
int launch_scan_examples_nq(css_index* ix, const Rows& rows, const float* epad, int k, const ExampleArgs& ea, int* gthr,
                            const SweepGeom& sg, hipStream_t st) {
    return sweep_variant(ix, [&](auto TT, auto M) {
        return launch_scan_examples_t<NQ, decltype(TT)::value, decltype(M)::value>(ix, rows, epad, k, ea, gthr, sg, st);
    });
}

// The example sweep over the rows and the merge of its [block][k] part lists: the plain merge with ONE "query" at
// q0 = 0 (<L2>'s D = -key is f with its sign).
int search_examples_sweep(css_index* ix, const Rows& rows, int k, const ExampleArgs& ea, const SweepGeom& sg, float* D_dev,
                          int64_t* I_dev, hipStream_t st) {
    int* gthr = ix->gthr.p;
    hipLaunchKernelGGL(k_fill_int, dim3(1), dim3(64), 0, st, gthr, 1, host_f2key(-INFINITY));
    CSS_LAUNCH_CHECK();
    const float* epad = ix->qpad.p;
    const int rc = sweep_slots(ea.m, [&](auto NQ) {
        return launch_scan_examples_nq<decltype(NQ)::value>(ix, rows, epad, k, ea, gthr, sg, st);
    });
    return rc != CSS_OK ? rc : launch_merge_final(ix, rows, 0, 1, k, sg, D_dev, I_dev, st);
}

int merge_parts(const float* Dp, const int64_t* Ip, int nparts, int64_t stride_d, int64_t stride_i, int64_t nq, int k,
                int metric, float* D, int64_t* I, int device, void* stream, const char* who) {
    CSS_REQUIRE(Dp && Ip && D && I, "%s: NULL buffer", who);
    CSS_REQUIRE(nparts >= 1 && nq >= 0 && k >= 1 && k <= CSS_MAX_K, "%s: bad sizes", who);
    CSS_REQUIRE(metric == CSS_METRIC_IP || metric == CSS_METRIC_L2, "%s: unknown metric", who);
    int rc = css::check_device(device);
    if (rc != CSS_OK) return rc;
    if (nq == 0) return CSS_OK;
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps("knn_merge_parts", st);
    if (k > CSS_KERNEL_MAX_K) {
        if (metric == CSS_METRIC_IP)
            hipLaunchKernelGGL(k_merge_parts_rank<CSS_METRIC_IP>, dim3((unsigned)nq), dim3(256), 0, st, Dp, Ip, nparts, stride_d,
                               stride_i, nq, k, D, I);
        else
            hipLaunchKernelGGL(k_merge_parts_rank<CSS_METRIC_L2>, dim3((unsigned)nq), dim3(256), 0, st, Dp, Ip, nparts, stride_d,
                               stride_i, nq, k, D, I);
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    if (metric == CSS_METRIC_IP)
        hipLaunchKernelGGL(k_merge_parts<CSS_METRIC_IP>, dim3((unsigned)nq), dim3(64), 0, st, Dp, Ip, nparts, stride_d,
                           stride_i, nq, k, D, I);
    else
        hipLaunchKernelGGL(k_merge_parts<CSS_METRIC_L2>, dim3((unsigned)nq), dim3(64), 0, st, Dp, Ip, nparts, stride_d,
                           stride_i, nq, k, D, I);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Batches on an index WITHOUT bf16 shadow rows (more than ~38 M rows of 768 floats on one 288 GB GPU, or
// css_index_set_shadow(ix, 0)): the rows are rounded to bf16 one range at a time into a scratch buffer sized from
// the free HBM, every range is searched by the SAME cascade as a shadowed index (same error band: the scratch
// rows are exactly the shadow rows it would have had), and the per-range top-k lists are merged.  Per 10 M rows:
// 46 GB of conversion traffic + the 13.6 ms cascade, against 45-48 ms for the split-operand scan it replaces (three
// MFMA products per score, 4.4 x its algorithmic bytes), and the cost of the conversion is shared by up to 4096
// queries.  Returns kNoRangeScratch without touching the outputs (nothing enqueued) when no scratch of at least 2^20 rows can be had.
// (internal, never crosses the C ABI: "no scratch memory for the row ranges -- take the fallback"; distinct from every
// css_status so that an error of an inner launch can never be mistaken for it)
constexpr int kNoRangeScratch = 1;
int search_noshadow_ranges(css_index* ix, const Rows& rows, int64_t nq, int k, float* D_dev, int64_t* I_dev, hipStream_t st,
                           bool allow_i8) {
    int rc;
    const int64_t ntotal = rows.n;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return kNoRangeScratch;
    const size_t row_b = (size_t)ix->dpad * 2;
    int64_t rows_fit = (int64_t)((free_b + ix->xh_tmp.cap * 2) / 2 / row_b);          // half of what is free (incl. our own scratch)
    rows_fit = std::min<int64_t>(rows_fit, 16ll << 20) / CZ_T * CZ_T;
    int64_t S = std::min<int64_t>((ntotal + CZ_T - 1) / CZ_T * CZ_T, rows_fit);
    if (S < std::min<int64_t>(ntotal, 1ll << 20)) return kNoRangeScratch;
    if (ix->range_rows > 0) S = std::min<int64_t>(S, (ix->range_rows + CZ_T - 1) / CZ_T * CZ_T);
    // int8 scratch rows where the int8 scan pays (38 GB of conversion traffic per 10 M rows instead of 46, half the scan):
    // same quantiser as k_ingest_rows, whose running maximum of the int8 error norms covers every row of the index
    // (allow_i8 = false: an index with int8 rows of its own whose int8 choice was already declined for this search)
    const bool use_i8 = allow_i8 && batch_i8_wanted(ix, k, std::min<int64_t>(S, ntotal), nq);
    if (use_i8 && (rc = ix->x8s_tmp.grow((size_t)S + 256)) != CSS_OK) return rc;
    if (!ix->xh_tmp.try_exact((size_t)S * ix->dpad)) return kNoRangeScratch;   // (exact size: grow() would double a multi-GB buffer)
    const int nranges = (int)((ntotal + S - 1) / S);
    float* Dp = D_dev;
    int64_t* Ip = I_dev;
    // (nothing enqueued yet: the fallback is safe)
    if (nranges > 1 && !try_exact_pair(ix->rng_d, ix->rng_i, (size_t)nranges * nq * k)) return kNoRangeScratch;
    ProfScope all("knn_noshadow_ranges", st);
    for (int r = 0; r < nranges; ++r) {
        const int64_t row0 = (int64_t)r * S, n = std::min<int64_t>(S, ntotal - row0);
        if (use_i8) {
            ProfScope ps("knn_rows_to_i8", st);
            const float* src_ = rows.xb + (size_t)row0 * ix->dpad;
            signed char* dst_ = reinterpret_cast<signed char*>(ix->xh_tmp.p);
            const dim3 grid_((unsigned)((n + 3) / 4));
            switch (ix->dpad) {   // (dpad % 256 == 0 and <= 1024: batch_i8_wanted)
                case 256: hipLaunchKernelGGL(k_rows_to_i8_wide<4>, grid_, dim3(256), 0, st, src_, dst_, ix->x8s_tmp.p, n); break;
                case 512: hipLaunchKernelGGL(k_rows_to_i8_wide<8>, grid_, dim3(256), 0, st, src_, dst_, ix->x8s_tmp.p, n); break;
                case 768: hipLaunchKernelGGL(k_rows_to_i8_wide<12>, grid_, dim3(256), 0, st, src_, dst_, ix->x8s_tmp.p, n); break;
                default: hipLaunchKernelGGL(k_rows_to_i8_wide<16>, grid_, dim3(256), 0, st, src_, dst_, ix->x8s_tmp.p, n); break;
            }
            CSS_LAUNCH_CHECK();
        } else {
            ProfScope ps("knn_rows_to_bf16", st);
            const int64_t n8 = n * ix->dpad / 8;   // (dpad is a multiple of 64)
            const unsigned blocks = (unsigned)std::min<int64_t>((n8 + 255) / 256, (int64_t)ix->num_cus * 64);
            hipLaunchKernelGGL(k_rows_to_bf16_x8, dim3(blocks), dim3(256), 0, st, rows.xb + (size_t)row0 * ix->dpad, ix->xh_tmp.p, n8);
            CSS_LAUNCH_CHECK();
        }
        if (nranges > 1) {
            Dp = ix->rng_d.p + (size_t)r * nq * k;
            Ip = ix->rng_i.p + (size_t)r * nq * k;
        }
        const Rows sub = rows.range(row0, n, ix->dpad, use_i8 ? nullptr : ix->xh_tmp.p,
                                    use_i8 ? reinterpret_cast<const unsigned char*>(ix->xh_tmp.p) : nullptr,
                                    use_i8 ? ix->x8s_tmp.p : nullptr);
        SweepGeom sg;
        if ((rc = make_sweep_geom(ix, sub, k, &sg)) != CSS_OK) return rc;
        const int chunk = coarse_max_chunk(ix);
        for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
            const int nqc = (int)std::min<int64_t>(chunk, nq - q0);
            if ((rc = launch_scan_coarse(ix, sub, (int)q0, nqc, k, Dp, Ip, st, sg, CascadeKind::Batch, use_i8,
                                         r == nranges - 1 && q0 + nqc == nq)) != CSS_OK) return rc;
        }
    }
    if (nranges > 1)
        return merge_parts(ix->rng_d.p, ix->rng_i.p, nranges, nq * k, nq * k, nq, k, ix->metric, D_dev, I_dev, ix->device, st,
                           "css_index_search");
    return CSS_OK;
}

// RAII: one turn at the shared workspaces for what the caller enqueues on `st`.  The previous turn may still be
// running on another stream and owns the workspaces until its event: wait for it (a turn on the same stream is
// ordered already).  The end of the scope records the event for the next turn -- also after a failed enqueue, because
// whatever was launched before the error still uses the workspaces -- and when that cannot be recorded the device is
// drained instead.  Turns nest (search_any_k around search_dev_locked): the outermost record is the last.  Caller
// holds ws_mu, and returns `rc` when it is not CSS_OK.
struct WsTurn {
    css_index* ix;
    hipStream_t st;
    int rc = CSS_OK;
    WsTurn(css_index* i, hipStream_t s) : ix(i), st(s) {
        if (!(ix->ws_pending && ix->ws_stream != st)) return;
        const hipError_t e = hipStreamWaitEvent(st, ix->ws_ev, 0);
        if (e != hipSuccess) rc = css::hip_fail(e, "hipStreamWaitEvent(st, ix->ws_ev, 0)", __FILE__, __LINE__);
    }
    WsTurn(const WsTurn&) = delete;
    ~WsTurn() {
        if (hipEventRecord(ix->ws_ev, st) == hipSuccess) {
            ix->ws_stream = st;
            ix->ws_pending = true;
        } else {
            (void)hipDeviceSynchronize();
            ix->ws_pending = false;
        }
    }
};

// The lock and device frame of every search entry point, host or `_dev`: the shared lock on mu, ws_mu, the rows as a
// value (mask_dev: the device allow-bitmap of a `_dev` call) and the index's device made current.  on_empty = false
// leaves the device alone when the index has no rows (css_index_range_search answers that without one).
struct CallScope {
    css_index* ix;
    std::shared_lock<std::shared_mutex> lk;
    std::lock_guard<std::mutex> wl;
    Rows rows;
    std::optional<DeviceGuard> dev;
    explicit CallScope(css_index* i, const uint32_t* mask_dev = nullptr, bool on_empty = true)
        : ix(i), lk(i->mu), wl(i->ws_mu), rows(rows_of(i, mask_dev)) {
        if (on_empty || rows.n > 0) dev.emplace(i->device);
    }
};

// the score of an output slot that no row fills: the worst of the metric
inline float pad_score(const css_index* ix) { return ix->metric == CSS_METRIC_IP ? -FLT_MAX : FLT_MAX; }

// `nrows` output rows of k entries each put in best-first order (score, then id)
int launch_sort_rows(css_index* ix, float* D, int64_t* I, int64_t nrows, int k, hipStream_t st) {
    if (ix->metric == CSS_METRIC_IP) hipLaunchKernelGGL(k_sort_rows<CSS_METRIC_IP>, dim3((unsigned)nrows), dim3(1024), 0, st, D, I, k);
    else hipLaunchKernelGGL(k_sort_rows<CSS_METRIC_L2>, dim3((unsigned)nrows), dim3(1024), 0, st, D, I, k);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// Query prep of every search: the row kernel of ingest (normalise, zero pad, squared norm) from raw [nq, dim] rows
// into qpad / qnorm2 rows row0.. (the example table of css_index_search_examples is prepared in segments), and
// ||q - bf16(q)||^2 into `qerr2` where the caller keeps it.
int prep_queries(css_index* ix, const float* src, int64_t nq, int normalize_q, float* qerr2, hipStream_t st, int64_t row0 = 0) {
    hipLaunchKernelGGL(k_ingest_rows<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, src,
                       ix->qpad.p + (size_t)row0 * ix->dpad, ix->qnorm2.p + row0, nq, ix->dim, ix->dpad, normalize_q, 0ull, 0ll, (unsigned short*)nullptr, (int*)nullptr, qerr2,
                       (unsigned char*)nullptr, (float*)nullptr);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// q_dev: raw [nq, dim] device queries.  Caller holds ws_mu and a shared lock on mu.
int search_dev_enqueue(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, int normalize_q, float* D_dev,
                       int64_t* I_dev, hipStream_t st);
int search_dev_locked(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, int normalize_q, float* D_dev,
                      int64_t* I_dev, hipStream_t st) {
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    return search_dev_enqueue(ix, rows, q_dev, nq, k, normalize_q, D_dev, I_dev, st);
}
int search_dev_enqueue(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, int normalize_q, float* D_dev,
                       int64_t* I_dev, hipStream_t st) {
    CSS_REQUIRE(k >= 1 && k <= CSS_MAX_K, "css_index_search: k=%d outside [1, %d]", k, CSS_MAX_K);
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search: nq=%lld out of range", (long long)nq);
    if (nq == 0) return CSS_OK;
    const KnnEnv& env = knn_env();
    int rc;
    // rows appended on another stream (css_index_add_dev / _add_synthetic) must have landed
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->qpad.grow((size_t)(nq + 256) * ix->dpad)) != CSS_OK) return rc;
    if ((rc = ix->qnorm2.grow((size_t)nq + 256)) != CSS_OK) return rc;
    if ((rc = ix->qerr2.grow((size_t)nq + 256)) != CSS_OK) return rc;
    // (int8 rows: the int8 queries' error norms of every chunk of this search -- never reallocated between two chunks)
    if (rows.x8 != nullptr && (rc = ix->qerr2_i8.grow((size_t)nq + 256)) != CSS_OK) return rc;
    if ((rc = ix->gthr.grow((size_t)nq + 256)) != CSS_OK) return rc;
    // 1..4 queries through the sweep cascade: its init launch prepares the query rows as well (one launch less in front
    // of a 1.4 ms search).  Which shadow rows a search reads is decided once (the per-index int8 feedback counts searches).
    // 3 or 4 queries are VALU-bound in that sweep (10 M rows: 2.65 ms at k = 10): they, and up to 16 queries, sweep on the
    // int8 MFMA where that applies (mfma_sweep_applies); where not, 3 or 4 queries are sooner through the int8 scan of
    // batches from 3 M rows on (1.98 ms; 1 M rows: sweep 0.34 vs scan 0.39 ms; k = 100 goes through the bf16 scan, 3.2 ms
    // against the sweep's 2.8-2.9); two queries always sweep (1.36 vs 1.93 ms).  One session.
    const bool i8_scan_ok = rows.x8 != nullptr && ix->metric == CSS_METRIC_IP && ix->dpad % 256 == 0 && ix->dpad <= 1024 &&
                            env.batch_i8 != 0;
    const bool mfma_sweep_ok = mfma_sweep_applies(ix, rows, nq, k);
    const int sweep_max = (k <= 32 && rows.n >= 3000000 && i8_scan_ok) ? 2 : 4;   // VALU sweep
    const bool sweep_base = rows.n > 0 && k <= CSS_KERNEL_MAX_K && (rows.xh != nullptr || rows.x8 != nullptr) &&
                            (ix->search_mode == CSS_SEARCH_COARSE ||
                             (ix->search_mode == CSS_SEARCH_AUTO && (nq > 4 || k > 32 || rows.n >= 100000)));
    const bool sweep_i8 = sweep_base && rows.x8 != nullptr && (nq <= sweep_max || mfma_sweep_ok) && sweep_uses_i8(ix, rows);
    const bool sweep_path = sweep_base && ((mfma_sweep_ok && sweep_i8) || (nq <= sweep_max && (sweep_i8 || rows.xh != nullptr)));
    if (!sweep_path && (rc = prep_queries(ix, q_dev, nq, normalize_q, ix->qerr2.p, st)) != CSS_OK) return rc;
    if (rows.n == 0) {
        const int64_t n = nq * k;
        hipLaunchKernelGGL(k_fill_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D_dev, I_dev, n, pad_score(ix));
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    CSS_REQUIRE(k <= CSS_KERNEL_MAX_K, "css_index_search: internal: k=%d reached the scan kernels (limit %d)", k, CSS_KERNEL_MAX_K);
    SweepGeom sg;
    if ((rc = make_sweep_geom(ix, rows, k, &sg)) != CSS_OK) return rc;

    const int mode = ix->search_mode;
    const bool batch_ok = nq > 16 && k <= kMfmaMaxK && ix->dpad % MF_BK == 0;  // the MFMA scan kernels apply
    // Where the candidate path answers sooner than the exact fp32 kernels (tools/knn_crossover.py on MI355X, 768-d, ms
    // candidate / exact): 5..16 queries at every size (2 k rows 0.07 / 0.15, 100 k 0.16 / 0.28, 1 M 0.44 / 0.93); 1..4
    // queries with the reference's k' = 100 at every size too (2 k 0.065 / 0.134, 100 k 0.13 / 0.17, 1 M 0.32 / 0.66:
    // the exact kernels keep k-entry lists per block), with k = 10 from ~100 k rows on (50 k 0.093 / 0.074, 100 k
    // 0.099 / 0.119, 1 M 0.25 / 0.64).  Round 2 switched at 1.2 M / 0.4 M rows: the cascade has since lost most of its
    // fixed cost and the few-query sweep reads int8 rows.
    const bool coarse_pays = nq > 4 || k > 32 || rows.n >= 100000;
    const bool want_split = mode == CSS_SEARCH_SPLIT;   // split-operand candidate scan from the fp32 rows
    const bool want_candidates = mode == CSS_SEARCH_COARSE || (mode == CSS_SEARCH_AUTO && coarse_pays);
    // Which shadow rows this search reads is decided HERE, once (the per-index int8 feedback counts searches, not chunks).
    // An index with int8 rows only takes the candidate path where the int8 rows are chosen; otherwise it goes on like an
    // index without shadow rows (bf16 scratch ranges for batches, the exact kernels for a few queries).
    if (want_candidates && (rows.xh != nullptr || rows.x8 != nullptr)) {
        const bool sweep = sweep_path;
        const bool use_i8 = rows.x8 != nullptr && (sweep ? sweep_i8 : batch_i8_wanted(ix, k, rows.n, nq));
        if (use_i8 || rows.xh != nullptr) {
            // (3..32 queries on int8 rows where mfma_sweep_applies: the sweep on the int8 MFMA, int8 queries too)
            const CascadeKind kind = !sweep ? CascadeKind::Batch : ((use_i8 && mfma_sweep_ok) ? CascadeKind::SweepMfma : CascadeKind::SweepValu);
            if (sweep) return launch_scan_coarse(ix, rows, 0, (int)nq, k, D_dev, I_dev, st, sg, kind, use_i8, true, q_dev, normalize_q);
            const int chunk = coarse_max_chunk(ix);
            for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
                const int nqc = (int)std::min<int64_t>(chunk, nq - q0);
                if ((rc = launch_scan_coarse(ix, rows, (int)q0, nqc, k, D_dev, I_dev, st, sg, kind, use_i8, q0 + nqc == nq)) != CSS_OK)
                    return rc;
            }
            return CSS_OK;
        }
    }
    // no shadow rows: batches take the same cascade over bf16 rows rounded on the fly, one row range at a time
    // (a k beyond the MFMA kernels, or no HBM left for the scratch rows: the split-operand scan)
    if (want_candidates && rows.xh == nullptr && nq > 16 && ix->dpad % 128 == 0) {
        rc = search_noshadow_ranges(ix, rows, nq, k, D_dev, I_dev, st, rows.x8 == nullptr);
        if (rc != kNoRangeScratch) return rc;
    }
    if (batch_ok && k + kSplitExtra <= kMfmaMaxK && (want_split || (want_candidates && rows.xh == nullptr))) {
        for (int64_t q0 = 0; q0 < nq; q0 += 4096) {   // (chunked like the bf16 cascade: candidate buffers are per query)
            const int nqc = (int)std::min<int64_t>(4096, nq - q0);
            rc = ix->metric == CSS_METRIC_IP ? launch_scan_split_rescore<CSS_METRIC_IP>(ix, rows, (int)q0, nqc, k, D_dev, I_dev, sg, st)
                                             : launch_scan_split_rescore<CSS_METRIC_L2>(ix, rows, (int)q0, nqc, k, D_dev, I_dev, sg, st);
            if (rc != CSS_OK) return rc;
        }
        return CSS_OK;
    }
    // shadow-less batches whose k leaves no room for the split scan's extra ranks (k = 61 .. 64): the fp32-input MFMA
    // scan, not 16-query VALU sweeps
    if (batch_ok && (want_split || (want_candidates && rows.xh == nullptr))) {
        return ix->metric == CSS_METRIC_IP ? launch_scan_fp32mfma<CSS_METRIC_IP>(ix, rows, (int)nq, k, D_dev, I_dev, st)
                                           : launch_scan_fp32mfma<CSS_METRIC_L2>(ix, rows, (int)nq, k, D_dev, I_dev, st);
    }
    // exact fp32 arithmetic inside the scan: fp32-input MFMA for batches, VALU sweeps for up to 16 queries
    if (batch_ok && mode == CSS_SEARCH_EXACT_FP32) {
        return ix->metric == CSS_METRIC_IP ? launch_scan_fp32mfma<CSS_METRIC_IP>(ix, rows, (int)nq, k, D_dev, I_dev, st)
                                           : launch_scan_fp32mfma<CSS_METRIC_L2>(ix, rows, (int)nq, k, D_dev, I_dev, st);
    }
    if ((rc = grow_part(ix, (size_t)sg.nq_sweep * sg.G * k)) != CSS_OK) return rc;
    for (int64_t q0 = 0; q0 < nq; q0 += sg.nq_sweep) {
        const int nqc = (int)std::min<int64_t>(sg.nq_sweep, nq - q0);
        if ((rc = search_chunk_small(ix, rows, (int)q0, nqc, k, sg, D_dev, I_dev, st)) != CSS_OK) return rc;
    }
    return CSS_OK;
}


}  // namespace

extern "C" {

int css_index_create(int dim, int metric, int device, css_index** out) {
    CSS_REQUIRE(out != nullptr, "css_index_create: out is NULL");
    CSS_REQUIRE(dim >= 1 && dim <= 8192, "css_index_create: dim=%d outside [1, 8192]", dim);
    CSS_REQUIRE(metric == CSS_METRIC_IP || metric == CSS_METRIC_L2, "css_index_create: unknown metric %d", metric);
    int rc = css::check_device(device);
    if (rc != CSS_OK) return rc;
    DeviceGuard g(device);
    css_index* ix = new css_index();
    ix->dim = dim;
    ix->dpad = (dim + 63) / 64 * 64;
    ix->metric = metric;
    ix->device = device;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) == hipSuccess) ix->num_cus = p.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ix;
        return css::hip_fail(e, "hipStreamCreate", __FILE__, __LINE__);
    }
    e = hipEventCreateWithFlags(&ix->ws_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(ix->stream);
        delete ix;
        return css::hip_fail(e, "hipEventCreate", __FILE__, __LINE__);
    }
    e = hipEventCreateWithFlags(&ix->ingest_ev, hipEventDisableTiming);
    if (e == hipSuccess && !ix->maxn2.try_exact(3)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemset(ix->maxn2.p, 0, 3 * sizeof(int));
    // (null-stream memset vs the non-blocking streams every later launch uses: order it here, once)
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (ix->ingest_ev) (void)hipEventDestroy(ix->ingest_ev);
        if (ix->ws_ev) (void)hipEventDestroy(ix->ws_ev);
        (void)hipStreamDestroy(ix->stream);
        delete ix;
        return css::hip_fail(e, "hipMalloc(maxn2)", __FILE__, __LINE__);
    }
    *out = ix;
    return CSS_OK;
}

int css_index_free(css_index* ix) {
    if (!ix) return CSS_OK;
    DeviceGuard g(ix->device);
    (void)hipStreamSynchronize(ix->stream);
    if (ix->ingest_pending) (void)hipEventSynchronize(ix->ingest_ev);
    for (css_index::I8Feedback* f : {&ix->fb_batch, &ix->fb_sweep})
        if (f->h_nflag) {   // (the count of the last int8 search may still be on its way)
            (void)hipDeviceSynchronize();
            (void)hipEventDestroy(f->ev);
            (void)hipHostFree(f->h_nflag);
        }
    if (ix->h_stage) (void)hipHostFree(ix->h_stage);
    if (ix->ingest_ev) (void)hipEventDestroy(ix->ingest_ev);
    if (ix->ws_ev) (void)hipEventDestroy(ix->ws_ev);
    (void)hipStreamDestroy(ix->stream);
    // the row storage and every workspace by their DevBufs, inside the DeviceGuard: they free on the index's device
    // (hipFree waits for the device: nothing enqueued by a _dev call still runs)
    delete ix;
    return CSS_OK;
}

namespace {
// the index is again one that never received terms; caller holds mu exclusively and the stream is idle
int drop_terms(css_index* ix) {
    ix->lex_rows = 0;
    ix->lex_off_h.clear();
    CSS_HIP_TRY(ix->lex_ent.drop());
    CSS_HIP_TRY(ix->lex_dl.drop());
    CSS_HIP_TRY(ix->lex_off.drop());
    CSS_HIP_TRY(ix->lex_df.drop());
    CSS_HIP_TRY(ix->lex_total.drop());
    return CSS_OK;
}
// ... and one that never received sparse vectors
int drop_sparse(css_index* ix) {
    ix->sp_rows = 0;
    ix->sp_off_h.clear();
    CSS_HIP_TRY(ix->sp_ent.drop());
    CSS_HIP_TRY(ix->sp_off.drop());
    return CSS_OK;
}
// ... and one that never received token matrices
int drop_tokens(css_index* ix) {
    ix->tk_rows = 0;
    ix->tk_dim = 0;
    ix->tk_off_h.clear();
    CSS_HIP_TRY(ix->tk_tok.drop());
    CSS_HIP_TRY(ix->tk_code.drop());   // (the codec itself stays)
    CSS_HIP_TRY(ix->tk_res.drop());
    CSS_HIP_TRY(ix->tk_off.drop());
    return CSS_OK;
}
}  // namespace

int css_index_reset(css_index* ix) {
    CSS_REQUIRE(ix, "css_index_reset: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    set_ntotal(ix, 0);
    if (!ix->xh.p) ix->shadow = -1;
    DeviceGuard g(ix->device);
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ingest_ev, 0));
    if (ix->ws_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ws_ev, 0));   // a search enqueued on another stream still reads maxn2
    CSS_HIP_TRY(hipMemsetAsync(ix->maxn2.p, 0, 3 * sizeof(int), ix->stream));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    // the columns go with the rows: the index is again one that never set any
    for (RowColumn* col : ix->columns()) CSS_HIP_TRY(col->words.drop());
    for (AttrColumn& a : ix->attrs) a.type = -1;
    int rc = drop_terms(ix);   // and the term lists with their statistics, the sparse vectors and the token matrices
    if (rc == CSS_OK) rc = drop_sparse(ix);
    return rc != CSS_OK ? rc : drop_tokens(ix);
}

namespace {
// The compaction proper (css_index_remove_rows): rows [first, n) of which `kept - first` survive.  Everything is
// enqueued on the index's stream; the caller waits for it.  Host memory read by the copies (keep, *patch) stays
// valid until then.
int compact_rows(css_index* ix, const uint32_t* keep, int64_t n, int64_t first, uint32_t* patch) {
    const hipStream_t st = ix->stream;
    const int dpad = ix->dpad;
    int rc;
    // the rows below the first removed one stay: one read for the maxima
    for (int64_t c0 = 0; c0 < first; c0 += kCompactWindowRows) {
        const int64_t nc = std::min(kCompactWindowRows, first - c0);
        hipLaunchKernelGGL(k_rows_maxima, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, ix->xb.p + (size_t)c0 * dpad, nc, ix->dim,
                           dpad, ix->maxn2.p);
        CSS_LAUNCH_CHECK();
    }
    // bounce rows: what 64 MiB hold, a whole number of keep words, never more than one launch covers
    // (and never more than the rows that can move)
    const int64_t W = std::min<int64_t>({kCompactWindowRows, std::max<int64_t>(32, ((64ll << 20) / ((int64_t)dpad * 4)) / 32 * 32),
                                         (int64_t)((n - (first & ~31ll) + 31) / 32 * 32)});
    const int64_t words = (n + 31) / 32;
    const size_t need_words = (size_t)std::min<int64_t>(kCompactWords, words);
    if ((rc = ix->compact_bits.grow_exact(need_words, "hipMalloc(compaction bitmap)")) != CSS_OK) return rc;
    if ((rc = ix->compact_pre.grow_exact(need_words, "hipMalloc(compaction bitmap)")) != CSS_OK) return rc;
    const uint32_t tail_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu;
    int64_t s0 = first & ~31ll;   // windows start on a keep word
    int64_t dnext = first;        // next free slot
    // the word that holds the first removed row: its lower rows stay where they are and are not part of the move
    *patch = keep[first >> 5] & ~((1u << (first & 31)) - 1u);
    while (s0 < n) {
        const int64_t src0 = std::max(s0, first);
        const int64_t gap = src0 - dnext;   // free slots below the window's first source row
        // gap >= L: every destination of the window lies below its sources whatever the bits are
        int64_t L = gap >= W ? std::min(gap / 32 * 32, kCompactWindowRows) : W;
        L = std::min(L, n - s0);
        const int64_t w0 = s0 >> 5, nw = (L + 31) / 32;
        int64_t surv = 0;
        for (int64_t w = 0; w < nw; ++w) {
            uint32_t v = (w0 + w == (first >> 5)) ? *patch : keep[w0 + w];
            if (w0 + w == words - 1) v &= tail_mask;
            surv += __builtin_popcount(v);
        }
        if (surv > 0) {
            CSS_HIP_TRY(hipMemcpyAsync(ix->compact_bits.p, keep + w0, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            if (w0 == (first >> 5))
                CSS_HIP_TRY(hipMemcpyAsync(ix->compact_bits.p, patch, sizeof(uint32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_keep_prefix, dim3(1), dim3(1024), 0, st, ix->compact_bits.p, ix->compact_pre.p, (int)nw);
            CSS_LAUNCH_CHECK();
            const unsigned blocks = (unsigned)((L + 3) / 4);
            float* dst = ix->xb.p + (size_t)dnext * dpad;
            unsigned short* dh = ix->xh.p ? ix->xh.p + (size_t)dnext * dpad : nullptr;
            unsigned char* d8 = ix->x8.p ? ix->x8.p + (size_t)dnext * dpad : nullptr;
            float* d8s = ix->x8.p ? ix->x8s.p + dnext : nullptr;
            const float* src = ix->xb.p + (size_t)s0 * dpad;
            if (dnext + surv <= src0) {   // destinations wholly below the sources: straight into place
                hipLaunchKernelGGL(k_compact_rows, dim3(blocks), dim3(256), 0, st, ix->compact_bits.p, ix->compact_pre.p, L, src, dst,
                                   ix->xnorm2.p + dnext, ix->dim, dpad, dh, ix->maxn2.p, d8, d8s);
                CSS_LAUNCH_CHECK();
            } else {                      // they overlap: through the scratch rows, the kernel boundary orders read and overwrite
                if ((rc = ix->stage.grow((size_t)W * dpad)) != CSS_OK) return rc;
                hipLaunchKernelGGL(k_compact_gather, dim3(blocks), dim3(256), 0, st, ix->compact_bits.p, ix->compact_pre.p, L, src,
                                   ix->stage.p, dpad);
                CSS_LAUNCH_CHECK();
                hipLaunchKernelGGL(k_compact_rows, dim3((unsigned)((surv + 3) / 4)), dim3(256), 0, st, (const uint32_t*)nullptr,
                                   (const uint32_t*)nullptr, surv, ix->stage.p, dst, ix->xnorm2.p + dnext, ix->dim, dpad, dh, ix->maxn2.p,
                                   d8, d8s);
                CSS_LAUNCH_CHECK();
            }
        }
        dnext += surv;
        s0 += L;
    }
    return CSS_OK;
}

// A column (moved as bits, whatever it holds) through the same keep bits, OUT OF PLACE into `dst` (column_alloc: at
// the column's default beforehand): a second 4-byte-per-row
// buffer has none of the overlap hazards of the row windows above, and the caller swaps it in.  Enqueued behind
// compact_rows on the index's stream (it reuses compact_bits / compact_pre); `keep` stays valid until the caller waited.
int compact_column(css_index* ix, const uint32_t* keep, int64_t n, const RowColumn& col, const DevBuf<int32_t>& to) {
    const int32_t* src = col.words.p;
    int32_t* dst = to.p;
    const hipStream_t st = ix->stream;
    const int64_t words = (n + 31) / 32;
    const uint32_t tail_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu;
    const size_t need_words = (size_t)std::min<int64_t>(kCompactWords, words);
    int rc;
    if ((rc = ix->compact_bits.grow_exact(need_words, "hipMalloc(compaction bitmap)")) != CSS_OK) return rc;
    if ((rc = ix->compact_pre.grow_exact(need_words, "hipMalloc(compaction bitmap)")) != CSS_OK) return rc;
    int64_t dnext = 0;
    for (int64_t s0 = 0; s0 < n; s0 += kCompactWindowRows) {
        const int64_t L = std::min(kCompactWindowRows, n - s0);
        const int64_t w0 = s0 >> 5, nw = (L + 31) / 32;
        int64_t surv = 0;
        for (int64_t w = 0; w < nw; ++w) surv += __builtin_popcount(keep[w0 + w] & (w0 + w == words - 1 ? tail_mask : 0xFFFFFFFFu));
        if (surv > 0) {
            CSS_HIP_TRY(hipMemcpyAsync(ix->compact_bits.p, keep + w0, (size_t)nw * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_keep_prefix, dim3(1), dim3(1024), 0, st, ix->compact_bits.p, ix->compact_pre.p, (int)nw);
            CSS_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_compact_labels, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, st, ix->compact_bits.p,
                               ix->compact_pre.p, L, src + s0, dst + dnext);
            CSS_LAUNCH_CHECK();
        }
        dnext += surv;
    }
    return CSS_OK;
}

// a grid for the element-wise list kernels: enough blocks to fill the chip, never more than the elements need
inline unsigned lex_grid(const css_index* ix, int64_t count) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, (int64_t)ix->num_cus * 16));
}

// The term lists through the keep bits of css_index_remove_rows, OUT OF PLACE like compact_column: the new offsets are
// a host prefix sum over the mirror, k_lex_move moves the lists of the kept rows and takes those of the removed rows
// out of df and total_len.  Enqueued behind compact_rows on the index's stream; the caller waits, then commits.
struct TermCompaction {
    DevBuf<uint32_t> ent, dl, map;
    DevBuf<int64_t> off;
    std::vector<int64_t> off_h;   // (read by the copy until the caller has waited)
    std::vector<uint32_t> map_h;
    bool built = false;
    void commit(css_index* ix) {
        ix->lex_ent.swap(ent);
        ix->lex_dl.swap(dl);
        ix->lex_off.swap(off);
        ix->lex_off_h.swap(off_h);
        ix->lex_rows = (int64_t)ix->lex_off_h.size() - 1;
    }
};
int compact_terms(css_index* ix, const uint32_t* keep, TermCompaction* tc) {
    const int64_t T = ix->lex_rows;
    if (T == 0) return CSS_OK;
    const hipStream_t st = ix->stream;
    try {
        tc->map_h.resize((size_t)T);
        tc->off_h.assign(1, 0);
        for (int64_t r = 0; r < T; ++r) {
            if ((keep[r >> 5] >> (r & 31)) & 1u) {
                tc->map_h[(size_t)r] = (uint32_t)(tc->off_h.size() - 1);
                tc->off_h.push_back(tc->off_h.back() + (ix->lex_off_h[(size_t)r + 1] - ix->lex_off_h[(size_t)r]));
            } else {
                tc->map_h[(size_t)r] = kLexNoRow;
            }
        }
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_remove_rows: out of host memory");
        return CSS_ERR_OOM;
    }
    const size_t nT = tc->off_h.size() - 1;
    int rc;
    if ((rc = tc->ent.grow_exact(std::max<size_t>((size_t)tc->off_h.back(), 1), "hipMalloc(term lists)")) != CSS_OK) return rc;
    if ((rc = tc->dl.grow_exact(std::max<size_t>(nT, 1), "hipMalloc(term lists)")) != CSS_OK) return rc;
    if ((rc = tc->off.grow_exact(nT + 1, "hipMalloc(term lists)")) != CSS_OK) return rc;
    if ((rc = tc->map.grow_exact((size_t)T, "hipMalloc(term lists)")) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(tc->map.p, tc->map_h.data(), (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(tc->off.p, tc->off_h.data(), (nT + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lex_move, dim3((unsigned)((T + kWaves - 1) / kWaves)), dim3(256), 0, st, (const uint32_t*)ix->lex_ent.p,
                       (const int64_t*)ix->lex_off.p, (const uint32_t*)ix->lex_dl.p, (const uint32_t*)tc->map.p,
                       (const int64_t*)tc->off.p, T, tc->ent.p, tc->dl.p, ix->lex_df.p, ix->lex_total.p);
    CSS_LAUNCH_CHECK();
    tc->built = true;
    return CSS_OK;
}

// The sparse vectors through the same keep bits, OUT OF PLACE like compact_terms: a host prefix sum over the mirror, and
// k_sparse_move moves the vectors of the kept rows.  Enqueued on the index's stream; the caller waits, then commits.
struct SparseCompaction {
    DevBuf<unsigned long long> ent;
    DevBuf<uint32_t> map;
    DevBuf<int64_t> off;
    std::vector<int64_t> off_h;   // (read by the copy until the caller has waited)
    std::vector<uint32_t> map_h;
    bool built = false;
    void commit(css_index* ix) {
        ix->sp_ent.swap(ent);
        ix->sp_off.swap(off);
        ix->sp_off_h.swap(off_h);
        ix->sp_rows = (int64_t)ix->sp_off_h.size() - 1;
    }
};
int compact_sparse(css_index* ix, const uint32_t* keep, SparseCompaction* sc) {
    const int64_t T = ix->sp_rows;
    if (T == 0) return CSS_OK;
    const hipStream_t st = ix->stream;
    try {
        sc->map_h.resize((size_t)T);
        sc->off_h.assign(1, 0);
        for (int64_t r = 0; r < T; ++r) {
            if ((keep[r >> 5] >> (r & 31)) & 1u) {
                sc->map_h[(size_t)r] = (uint32_t)(sc->off_h.size() - 1);
                sc->off_h.push_back(sc->off_h.back() + (ix->sp_off_h[(size_t)r + 1] - ix->sp_off_h[(size_t)r]));
            } else {
                sc->map_h[(size_t)r] = kLexNoRow;
            }
        }
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_remove_rows: out of host memory");
        return CSS_ERR_OOM;
    }
    const size_t nT = sc->off_h.size() - 1;
    int rc;
    if ((rc = sc->ent.grow_exact(std::max<size_t>((size_t)sc->off_h.back(), 1), "hipMalloc(sparse vectors)")) != CSS_OK) return rc;
    if ((rc = sc->off.grow_exact(nT + 1, "hipMalloc(sparse vectors)")) != CSS_OK) return rc;
    if ((rc = sc->map.grow_exact((size_t)T, "hipMalloc(sparse vectors)")) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(sc->map.p, sc->map_h.data(), (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(sc->off.p, sc->off_h.data(), (nT + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sparse_move, dim3((unsigned)((T + kWaves - 1) / kWaves)), dim3(256), 0, st,
                       (const unsigned long long*)ix->sp_ent.p, (const int64_t*)ix->sp_off.p, (const uint32_t*)sc->map.p,
                       (const int64_t*)sc->off.p, T, sc->ent.p);
    CSS_LAUNCH_CHECK();
    sc->built = true;
    return CSS_OK;
}

// The token matrices through the same keep bits, OUT OF PLACE like compact_sparse, with k_tok_move_units.
struct TokenCompaction {
    DevBuf<unsigned short> tok, code;   // (a compressed store: code and res in place of tok)
    DevBuf<unsigned char> res;
    DevBuf<uint32_t> map;
    DevBuf<int64_t> off;
    std::vector<int64_t> off_h;   // (read by the copy until the caller has waited)
    std::vector<uint32_t> map_h;
    bool built = false;
    void commit(css_index* ix) {
        ix->tk_tok.swap(tok);
        ix->tk_code.swap(code);
        ix->tk_res.swap(res);
        ix->tk_off.swap(off);
        ix->tk_off_h.swap(off_h);
        ix->tk_rows = (int64_t)ix->tk_off_h.size() - 1;
    }
};
int compact_tokens(css_index* ix, const uint32_t* keep, TokenCompaction* tc) {
    const int64_t T = ix->tk_rows;
    if (T == 0) return CSS_OK;
    const hipStream_t st = ix->stream;
    try {
        tc->map_h.resize((size_t)T);
        tc->off_h.assign(1, 0);
        for (int64_t r = 0; r < T; ++r) {
            if ((keep[r >> 5] >> (r & 31)) & 1u) {
                tc->map_h[(size_t)r] = (uint32_t)(tc->off_h.size() - 1);
                tc->off_h.push_back(tc->off_h.back() + (ix->tk_off_h[(size_t)r + 1] - ix->tk_off_h[(size_t)r]));
            } else {
                tc->map_h[(size_t)r] = kLexNoRow;
            }
        }
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_remove_rows: out of host memory");
        return CSS_ERR_OOM;
    }
    const size_t nT = tc->off_h.size() - 1, P = (size_t)ix->tk_dim;
    int rc;
    const size_t nE = std::max<size_t>((size_t)tc->off_h.back(), 1), RB = P * (size_t)ix->tk_bits / 8;
    if (ix->tk_bits) {
        if ((rc = tc->code.grow_exact(nE, "hipMalloc(token codes)")) != CSS_OK) return rc;
        if ((rc = tc->res.grow_exact(nE * RB, "hipMalloc(token codes)")) != CSS_OK) return rc;
    } else if ((rc = tc->tok.grow_exact(nE * P, "hipMalloc(token matrices)")) != CSS_OK) {
        return rc;
    }
    if ((rc = tc->off.grow_exact(nT + 1, "hipMalloc(token matrices)")) != CSS_OK) return rc;
    if ((rc = tc->map.grow_exact((size_t)T, "hipMalloc(token matrices)")) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(tc->map.p, tc->map_h.data(), (size_t)T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CSS_HIP_TRY(hipMemcpyAsync(tc->off.p, tc->off_h.data(), (nT + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((T + kWaves - 1) / kWaves));
    if (ix->tk_bits) {   // the codes, 2 bytes a token, and the packed buckets, 4 to 64
        hipLaunchKernelGGL(k_tok_move_units<unsigned short>, grid, dim3(256), 0, st, (const unsigned short*)ix->tk_code.p,
                           (const int64_t*)ix->tk_off.p, (const uint32_t*)tc->map.p, (const int64_t*)tc->off.p, T, 1, tc->code.p);
        CSS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_tok_move_units<uint32_t>, grid, dim3(256), 0, st, reinterpret_cast<const uint32_t*>(ix->tk_res.p),
                           (const int64_t*)ix->tk_off.p, (const uint32_t*)tc->map.p, (const int64_t*)tc->off.p, T, (int)(RB / 4),
                           reinterpret_cast<uint32_t*>(tc->res.p));
    } else {
        hipLaunchKernelGGL(k_tok_move_units<uint4>, grid, dim3(256), 0, st, reinterpret_cast<const uint4*>(ix->tk_tok.p),
                           (const int64_t*)ix->tk_off.p, (const uint32_t*)tc->map.p, (const int64_t*)tc->off.p, T, (int)(P / 8),
                           reinterpret_cast<uint4*>(tc->tok.p));
    }
    CSS_LAUNCH_CHECK();
    tc->built = true;
    return CSS_OK;
}
}  // namespace

int css_index_remove_rows(css_index* ix, const uint32_t* keep_bits_host, int64_t* removed_out) {
    CSS_REQUIRE(ix && removed_out, "css_index_remove_rows: NULL argument");
    *removed_out = 0;
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);   // (stage, compact_bits / compact_pre, ws_pending)
    const int64_t n = ix->ntotal;
    if (n == 0) return CSS_OK;
    CSS_REQUIRE(keep_bits_host, "css_index_remove_rows: keep_bits is NULL");
    const int64_t words = (n + 31) / 32;
    const uint32_t tail_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu;
    int64_t first = -1, kept = 0;
    for (int64_t w = 0; w < words; ++w) {
        const uint32_t valid = w == words - 1 ? tail_mask : 0xFFFFFFFFu;
        const uint32_t v = keep_bits_host[w] & valid;
        kept += __builtin_popcount(v);
        if (first < 0 && v != valid) first = w * 32 + __builtin_ctz(~v & valid);
    }
    if (first < 0) return CSS_OK;   // nothing to remove: no device work
    DeviceGuard g(ix->device);
    // pending asynchronous adds, and searches on other streams that still read the rows and maxn2
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ingest_ev, 0));
    if (ix->ws_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ws_ev, 0));
    DevBuf<int32_t> ncol[css_index::kColumns];   // the compacted columns (only those that were set)
    const auto cols = ix->columns();
    int rc = CSS_OK;
    for (int c = 0; c < css_index::kColumns; ++c)
        if (cols[c]->words.p && kept > 0 && (rc = column_alloc(ix, *cols[c], ix->cap, &ncol[c])) != CSS_OK) return rc;
    TermCompaction tc;      // the compacted term lists (only where terms were set)
    SparseCompaction sc;    // the compacted sparse vectors (only where vectors were set)
    TokenCompaction kc;     // the compacted token matrices (only where matrices were set)
    CSS_HIP_TRY(hipMemsetAsync(ix->maxn2.p, 0, 3 * sizeof(int), ix->stream));
    uint32_t patch = 0;
    if (kept > 0) rc = compact_rows(ix, keep_bits_host, n, first, &patch);
    for (int c = 0; c < css_index::kColumns; ++c)
        if (rc == CSS_OK && ncol[c].p) rc = compact_column(ix, keep_bits_host, n, *cols[c], ncol[c]);
    if (rc == CSS_OK && ix->lex_df.p && kept > 0) rc = compact_terms(ix, keep_bits_host, &tc);
    if (rc == CSS_OK && !ix->sp_off_h.empty() && kept > 0) rc = compact_sparse(ix, keep_bits_host, &sc);
    if (rc == CSS_OK && !ix->tk_off_h.empty() && kept > 0) rc = compact_tokens(ix, keep_bits_host, &kc);
    // later adds and searches on any stream are ordered behind the compaction (as css_index_reset)
    const hipError_t e = hipStreamSynchronize(ix->stream);
    if (rc != CSS_OK) return rc;
    if (e != hipSuccess) return css::hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    for (int c = 0; c < css_index::kColumns; ++c)
        if (ncol[c].p) cols[c]->words.swap(ncol[c]);
    if (tc.built) tc.commit(ix);
    if (sc.built) sc.commit(ix);
    if (kc.built) kc.commit(ix);
    if (kept == 0 && (rc = drop_terms(ix)) != CSS_OK) return rc;   // emptied: as css_index_reset
    if (kept == 0 && (rc = drop_sparse(ix)) != CSS_OK) return rc;
    if (kept == 0 && (rc = drop_tokens(ix)) != CSS_OK) return rc;
    set_ntotal(ix, kept);
    if (kept == 0 && !ix->xh.p) ix->shadow = -1;   // emptied: as css_index_reset
    for (css_index::I8Feedback* f : {&ix->fb_batch, &ix->fb_sweep}) {   // (it described other rows; its copy has landed)
        f->pending = false;
        f->backoff = 0;
    }
    *removed_out = n - kept;
    return CSS_OK;
}

int css_index_bounds(css_index* ix, float out[3]) {
    CSS_REQUIRE(ix && out, "css_index_bounds: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    DeviceGuard g(ix->device);
    CSS_HIP_TRY(hipDeviceSynchronize());   // diagnostics: whichever stream the last add ran on
    CSS_HIP_TRY(hipMemcpy(out, ix->maxn2.p, 3 * sizeof(float), hipMemcpyDeviceToHost));
    return CSS_OK;
}

int css_index_reserve(css_index* ix, int64_t n) {
    CSS_REQUIRE(ix && n >= 0, "css_index_reserve: bad argument");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    if (n <= ix->cap) return CSS_OK;
    // exact-size allocation (no 1.5x growth): a 245 GB shard must not over-allocate
    return reallocate_rows(ix, n);
}

int css_index_ntotal(const css_index* ix, int64_t* n) {
    CSS_REQUIRE(ix && n, "css_index_ntotal: NULL argument");
    *n = ix->ntotal_pub.load();
    return CSS_OK;
}

int css_index_dim(const css_index* ix, int* dim) {
    CSS_REQUIRE(ix && dim, "css_index_dim: NULL argument");
    *dim = ix->dim;
    return CSS_OK;
}

int css_index_metric(const css_index* ix, int* metric) {
    CSS_REQUIRE(ix && metric, "css_index_metric: NULL argument");
    *metric = ix->metric;
    return CSS_OK;
}

int css_index_device(const css_index* ix, int* device) {
    CSS_REQUIRE(ix && device, "css_index_device: NULL argument");
    *device = ix->device;
    return CSS_OK;
}

int css_index_set_search_mode(css_index* ix, int mode) {
    CSS_REQUIRE(ix, "css_index_set_search_mode: NULL index");
    CSS_REQUIRE(mode == CSS_SEARCH_AUTO || mode == CSS_SEARCH_EXACT_FP32 || mode == CSS_SEARCH_COARSE || mode == CSS_SEARCH_SPLIT,
                "css_index_set_search_mode: unknown mode %d", mode);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->search_mode = mode;
    return CSS_OK;
}

int css_index_last_flagged(css_index* ix, int64_t* n) {
    CSS_REQUIRE(ix && n, "css_index_last_flagged: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    *n = 0;
    if (ix->last_nflag == nullptr) return CSS_OK;
    DeviceGuard g(ix->device);
    CSS_HIP_TRY(hipDeviceSynchronize());  // diagnostics: whichever stream the search ran on
    int v = 0;
    CSS_HIP_TRY(hipMemcpy(&v, ix->last_nflag, sizeof(int), hipMemcpyDeviceToHost));
    *n = v;
    return CSS_OK;
}

int css_index_set_range_rows(css_index* ix, int64_t rows) {
    CSS_REQUIRE(ix, "css_index_set_range_rows: NULL index");
    CSS_REQUIRE(rows >= 0, "css_index_set_range_rows: rows < 0");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->range_rows = rows;
    return CSS_OK;
}

int css_index_set_gram_rows(css_index* ix, int64_t rows) {
    CSS_REQUIRE(ix, "css_index_set_gram_rows: NULL index");
    CSS_REQUIRE(rows >= 0, "css_index_set_gram_rows: rows < 0");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->gram_rows = rows;
    return CSS_OK;
}

int css_index_set_sigterm_slots(css_index* ix, int slots) {
    CSS_REQUIRE(ix, "css_index_set_sigterm_slots: NULL index");
    CSS_REQUIRE(slots == -1 || slots == 0 || (slots >= 16 && slots <= kSigMaxSlots && (slots & (slots - 1)) == 0),
                "css_index_set_sigterm_slots: slots=%d is not -1, 0 or a power of two in [16, %d]", slots, kSigMaxSlots);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->sig_slots = slots;
    return CSS_OK;
}

int css_index_last_swept(css_index* ix, int64_t* n) {
    CSS_REQUIRE(ix && n, "css_index_last_swept: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    *n = 0;
    if (ix->last_nswept == nullptr) return CSS_OK;
    DeviceGuard g(ix->device);
    CSS_HIP_TRY(hipDeviceSynchronize());
    int v = 0;
    CSS_HIP_TRY(hipMemcpy(&v, ix->last_nswept, sizeof(int), hipMemcpyDeviceToHost));
    *n = v;
    return CSS_OK;
}

int css_index_shadow_info(css_index* ix, int* has_bf16, int* has_int8) {
    CSS_REQUIRE(ix && has_bf16 && has_int8, "css_index_shadow_info: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    const Rows rows = rows_of(ix);
    *has_bf16 = rows.xh != nullptr ? 1 : 0;
    *has_int8 = rows.x8 != nullptr ? 1 : 0;
    return CSS_OK;
}

int css_index_set_shadow(css_index* ix, int policy) {
    CSS_REQUIRE(ix, "css_index_set_shadow: NULL index");
    CSS_REQUIRE(policy >= -1 && policy <= 2, "css_index_set_shadow: policy %d outside {-1, 0, 1, 2}", policy);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    if (ix->ntotal != 0) {
        css::set_error("css_index_set_shadow: the index already holds %lld rows (set the policy on an empty index)",
                       (long long)ix->ntotal);
        return CSS_ERR_STATE;
    }
    DeviceGuard g(ix->device);
    ix->shadow_policy = policy;
    CSS_HIP_TRY(ix->xh.drop());   // start over: the next add decides again
    CSS_HIP_TRY(ix->x8.drop());
    CSS_HIP_TRY(ix->x8s.drop());
    ix->shadow = -1;
    return CSS_OK;
}

int css_index_set_id_base(css_index* ix, int64_t base) {
    CSS_REQUIRE(ix, "css_index_set_id_base: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->id_base = base;
    return CSS_OK;
}

int css_index_add(css_index* ix, const float* x_host, int64_t n, int normalize) {
    CSS_REQUIRE(ix, "css_index_add: NULL index");
    CSS_REQUIRE(n >= 0, "css_index_add: n < 0");
    if (n == 0) return CSS_OK;
    CSS_REQUIRE(x_host, "css_index_add: x is NULL");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    DeviceGuard g(ix->device);
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ingest_ev, 0));
    int rc = ensure_capacity(ix, ix->ntotal + n);
    if (rc != CSS_OK) return rc;
    // stage through a bounded device buffer so huge adds do not double the footprint
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)ix->dim * 4));
    if ((rc = ix->stage.grow((size_t)std::min(n, chunk) * ix->dim)) != CSS_OK) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        CSS_HIP_TRY(hipMemcpyAsync(ix->stage.p, x_host + (size_t)r0 * ix->dim, (size_t)m * ix->dim * 4,
                                   hipMemcpyHostToDevice, ix->stream));
        if ((rc = ingest(ix, ix->stage.p, m, normalize, false, 0, 0, ix->stream)) != CSS_OK) return rc;
        CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
        set_ntotal(ix, ix->ntotal + m);
    }
    return CSS_OK;
}

int css_index_add_dev(css_index* ix, const float* x_dev, int64_t n, int normalize, void* stream) {
    CSS_REQUIRE(ix, "css_index_add_dev: NULL index");
    CSS_REQUIRE(n >= 0, "css_index_add_dev: n < 0");
    if (n == 0) return CSS_OK;
    CSS_REQUIRE(x_dev, "css_index_add_dev: x is NULL");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    int rc = ensure_capacity(ix, ix->ntotal + n);
    if (rc != CSS_OK) return rc;
    // an earlier asynchronous add may have used another stream: chain it, so that the ONE event below covers it too
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ix->ingest_ev, 0));
    for (int64_t r0 = 0; r0 < n; r0 += (1ll << 30)) {
        const int64_t m = std::min<int64_t>(1ll << 30, n - r0);
        if ((rc = ingest(ix, x_dev + (size_t)r0 * ix->dim, m, normalize, false, 0, 0, (hipStream_t)stream)) != CSS_OK)
            return rc;
        set_ntotal(ix, ix->ntotal + m);
    }
    // the rows are written asynchronously on the caller's stream: later searches / reallocations / exports wait for this
    CSS_HIP_TRY(hipEventRecord(ix->ingest_ev, (hipStream_t)stream));
    ix->ingest_pending = true;
    return CSS_OK;
}

int css_index_add_synthetic(css_index* ix, int64_t n, uint64_t seed, int64_t first_row, int normalize,
                            void* stream) {
    CSS_REQUIRE(ix, "css_index_add_synthetic: NULL index");
    CSS_REQUIRE(n >= 0, "css_index_add_synthetic: n < 0");
    if (n == 0) return CSS_OK;
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    DeviceGuard g(ix->device);
    int rc = ensure_capacity(ix, ix->ntotal + n);
    if (rc != CSS_OK) return rc;
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ix->ingest_ev, 0));
    for (int64_t r0 = 0; r0 < n; r0 += (1ll << 30)) {
        const int64_t m = std::min<int64_t>(1ll << 30, n - r0);
        if ((rc = ingest(ix, nullptr, m, normalize, true, seed, first_row + r0, (hipStream_t)stream)) != CSS_OK)
            return rc;
        set_ntotal(ix, ix->ntotal + m);
    }
    CSS_HIP_TRY(hipEventRecord(ix->ingest_ev, (hipStream_t)stream));
    ix->ingest_pending = true;
    return CSS_OK;
}

int css_index_export(const css_index* cix, int64_t row0, int64_t n, float* x_out_host) {
    css_index* ix = const_cast<css_index*>(cix);
    CSS_REQUIRE(ix && x_out_host, "css_index_export: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    const Rows rows = rows_of(ix);
    CSS_REQUIRE(row0 >= 0 && n >= 0 && row0 + n <= rows.n, "css_index_export: rows [%lld, %lld) outside [0, %lld)",
                (long long)row0, (long long)(row0 + n), (long long)rows.n);
    if (n == 0) return CSS_OK;
    DeviceGuard g(ix->device);
    if (ix->ingest_pending) CSS_HIP_TRY(hipEventSynchronize(ix->ingest_ev));
    CSS_HIP_TRY(hipMemcpy2D(x_out_host, (size_t)ix->dim * 4, rows.xb + (size_t)row0 * ix->dpad, (size_t)ix->dpad * 4,
                            (size_t)ix->dim * 4, (size_t)n, hipMemcpyDeviceToHost));
    return CSS_OK;
}

namespace {
// Host entry points, all on the index's own stream.  The caller's allow-bitmap (one bit per row; null or an empty
// index: no mask) copied into mask_ws and made the mask of the call's rows:
int upload_allow_bits(css_index* ix, const uint32_t* bits_host, Rows* rows) {
    rows->mask = nullptr;
    if (!bits_host || rows->n == 0) return CSS_OK;
    const size_t words = (size_t)((rows->n + 31) / 32);
    int rc;
    if ((rc = ix->mask_ws.grow(words)) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(ix->mask_ws.p, bits_host, words * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
    rows->mask = ix->mask_ws.p;
    return CSS_OK;
}

// the device rows of a call's n = nq * k results in out_i: the ids at the front of the allocation, then their scores
int reserve_out(css_index* ix, size_t n, float** d_out, int64_t** i_out) {
    const int rc = ix->out_i.grow_exact(n * (sizeof(int64_t) + sizeof(float)), "hipMalloc(out_i)");
    if (rc != CSS_OK) return rc;
    *i_out = reinterpret_cast<int64_t*>(ix->out_i.p);
    *d_out = reinterpret_cast<float*>(*i_out + n);
    return CSS_OK;
}

// RAII: the frame of a host entry point around what it enqueues on the index's own stream.  The scope (CallScope)
// holds the locks, the device and the call's rows; upload() brings the caller's allow-bitmap and input over and
// reserves the result rows; finish() brings the results back.  Between the two the entry point enqueues its own
// search with `rows`, `d_out`, `i_out` (and `g_out`).  Input and results go through the pinned halves of h_stage
// (front: in, back: out) when BOTH fit kHostStage -- one copy and one wait, against a staging pass and a wait per
// pageable copy -- and directly otherwise.  The back half belongs to the scope only inside finish(): read_ints uses it
// in between.
extern "C++" {   // (upload is a template, and this part of the file is inside extern "C")
struct HostCall : CallScope {
    using CallScope::CallScope;
    static constexpr size_t kEntry = sizeof(int64_t) + sizeof(float);   // an [id | score] entry of out_i
    size_t n = 0;   // result entries
    float* d_out = nullptr;
    int64_t* i_out = nullptr;
    int32_t* g_out = nullptr;   // the trailing int32 column of the results, where the call has one
    int cols = 1;               // ... or `cols` of them, one after the other (set before upload)
    bool staged = false, enqueued = false;
    // the ONE size of a result entry: the staging decision and the offsets of the copy back both use it
    size_t record() const { return kEntry + (g_out ? cols * sizeof(int32_t) : 0); }

    // `count` elements from `src` into `dst`, the allow-bitmap (null: every row) into the mask of `rows`, and n_out
    // result entries reserved: [ids | scores] in out_i, their int32 column in `column` where the call names one
    template <typename T>
    int upload(const uint32_t* bits_host, DevBuf<T>& dst, const T* src, size_t count, size_t n_out = 0,
               DevBuf<int32_t>* column = nullptr) {
        int rc;
        n = n_out;
        if ((rc = dst.grow(count)) != CSS_OK) return rc;
        if (column) {
            if ((rc = column->grow(n * cols)) != CSS_OK) return rc;
            g_out = column->p;
        }
        if (n && (rc = reserve_out(ix, n, &d_out, &i_out)) != CSS_OK) return rc;
        const size_t bytes = count * sizeof(T);
        staged = css_index::fits_host_stage(bytes) && css_index::fits_host_stage(n * record());
        if (staged && ix->h_stage == nullptr)
            CSS_HIP_TRY(hipHostMalloc((void**)&ix->h_stage, 2 * css_index::kHostStage, hipHostMallocDefault));
        enqueued = true;
        if ((rc = upload_allow_bits(ix, bits_host, &rows)) != CSS_OK) return rc;
        const void* from = staged ? memcpy(ix->h_stage, src, bytes) : src;
        CSS_HIP_TRY(hipMemcpyAsync(dst.p, from, bytes, hipMemcpyHostToDevice, ix->stream));
        return CSS_OK;
    }
    // a failed call returns only when the stream is idle: the copies enqueued above read the caller's memory
    int wait_if_failed(int rc) {
        if (rc != CSS_OK && enqueued) (void)hipStreamSynchronize(ix->stream);
        return rc;
    }
    // rc: what upload() and the enqueue returned.  The results into the caller's D / I (and G: null, or a call
    // without the column, copies none); everything on the stream has finished when this returns.
    int finish(int rc, float* D_host, int64_t* I_host, int32_t* G_host = nullptr) {
        if (rc != CSS_OK) return wait_if_failed(rc);
        const hipStream_t st = ix->stream;
        if (!g_out) G_host = nullptr;
        if (staged) {   // one wait: [ids | scores] in one copy, and the column, into pinned memory
            char* back = ix->h_stage + css_index::kHostStage;
            CSS_HIP_TRY(hipMemcpyAsync(back, i_out, n * kEntry, hipMemcpyDeviceToHost, st));
            if (G_host) CSS_HIP_TRY(hipMemcpyAsync(back + n * kEntry, g_out, n * cols * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            CSS_HIP_TRY(hipStreamSynchronize(st));
            memcpy(I_host, back, n * sizeof(int64_t));
            memcpy(D_host, back + n * sizeof(int64_t), n * sizeof(float));
            if (G_host) memcpy(G_host, back + n * kEntry, n * cols * sizeof(int32_t));
            return CSS_OK;
        }
        CSS_HIP_TRY(hipMemcpyAsync(D_host, d_out, n * sizeof(float), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipMemcpyAsync(I_host, i_out, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (G_host) CSS_HIP_TRY(hipMemcpyAsync(G_host, g_out, n * cols * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipStreamSynchronize(st));
        return CSS_OK;
    }
};
}  // extern "C++"

// Any k in [1, CSS_MAX_K].  Up to CSS_KERNEL_MAX_K: one search.  Beyond: per query, ceil(k / CSS_KERNEL_MAX_K) passes of
// the SAME search paths, pass p over the allowed rows the passes before it did not return (exclusion bitmap), its
// results written straight into columns [p * 128, ..) of the query's output row; the comparator is total (score, then
// id), so the concatenation is the exact top-k, and one final sort puts entries whose scores came from different
// summation orders (fix-up sweep vs rescoring: <= 1e-6 apart) in order.  Everything is enqueued on `st`; nothing
// waits for the device.  Caller holds ws_mu and a shared lock on mu.
int search_any_k(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, int normalize_q, float* D_dev,
                 int64_t* I_dev, hipStream_t st) {
    CSS_REQUIRE(k >= 1 && k <= CSS_MAX_K, "css_index_search: k=%d outside [1, %d]", k, CSS_MAX_K);
    if (k <= CSS_KERNEL_MAX_K || rows.n == 0 || nq == 0)
        return search_dev_locked(ix, rows, q_dev, nq, k, normalize_q, D_dev, I_dev, st);
    CSS_REQUIRE(nq < (1 << 24), "css_index_search: nq=%lld out of range", (long long)nq);
    int rc;
    const int64_t words = (rows.n + 31) / 32;
    WsTurn turn(ix, st);   // excl_ws is a shared workspace, in use until the final sort is enqueued
    if (turn.rc != CSS_OK) return turn.rc;
    if ((rc = ix->excl_ws.grow((size_t)words)) != CSS_OK) return rc;
    Rows pass = rows;   // the same rows under the exclusion bitmap
    pass.mask = ix->excl_ws.p;
    for (int64_t q = 0; q < nq; ++q) {
        hipLaunchKernelGGL(k_mask_init, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, ix->excl_ws.p, rows.mask, words);
        CSS_LAUNCH_CHECK();
        for (int p = 0; p < k; p += CSS_KERNEL_MAX_K) {
            const int kk = std::min(CSS_KERNEL_MAX_K, k - p);
            float* Dq = D_dev + (size_t)q * k + p;
            int64_t* Iq = I_dev + (size_t)q * k + p;
            if ((rc = search_dev_locked(ix, pass, q_dev + (size_t)q * ix->dim, 1, kk, normalize_q, Dq, Iq, st)) != CSS_OK) return rc;
            if (p + kk < k) {
                hipLaunchKernelGGL(k_mask_clear, dim3(1), dim3(CSS_KERNEL_MAX_K), 0, st, ix->excl_ws.p, (const int64_t*)Iq, kk, rows.id_base);
                CSS_LAUNCH_CHECK();
            }
        }
    }
    return launch_sort_rows(ix, D_dev, I_dev, nq, k, st);
}
}  // namespace

int css_index_search_masked_dev(css_index* ix, const float* q_dev, int64_t nq, int k, int normalize_q,
                                const uint32_t* allow_bits_dev, float* D_dev, int64_t* I_dev, void* stream) {
    CSS_REQUIRE(ix, "css_index_search_dev: NULL index");
    CSS_REQUIRE(nq == 0 || (q_dev && D_dev && I_dev), "css_index_search_dev: NULL buffer");
    CallScope cs(ix, allow_bits_dev);
    return search_any_k(ix, cs.rows, q_dev, nq, k, normalize_q, D_dev, I_dev, (hipStream_t)stream);
}

int css_index_search_dev(css_index* ix, const float* q_dev, int64_t nq, int k, int normalize_q, float* D_dev,
                         int64_t* I_dev, void* stream) {
    return css_index_search_masked_dev(ix, q_dev, nq, k, normalize_q, nullptr, D_dev, I_dev, stream);
}

int css_index_search_masked(css_index* ix, const float* q_host, int64_t nq, int k, int normalize_q,
                            const uint32_t* allow_bits_host, float* D_host, int64_t* I_host) {
    CSS_REQUIRE(ix, "css_index_search: NULL index");
    CSS_REQUIRE(nq >= 0, "css_index_search: nq < 0");
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(q_host && D_host && I_host, "css_index_search: NULL buffer");
    CSS_REQUIRE(k >= 1 && k <= CSS_MAX_K, "css_index_search: k=%d outside [1, %d]", k, CSS_MAX_K);
    HostCall hc(ix);
    int rc = hc.upload(allow_bits_host, ix->q_raw, q_host, (size_t)nq * ix->dim, (size_t)nq * k);
    if (rc == CSS_OK) rc = search_any_k(ix, hc.rows, ix->q_raw.p, nq, k, normalize_q, hc.d_out, hc.i_out, ix->stream);
    return hc.finish(rc, D_host, I_host);
}

int css_index_search(css_index* ix, const float* q_host, int64_t nq, int k, int normalize_q, float* D_host,
                     int64_t* I_host) {
    return css_index_search_masked(ix, q_host, nq, k, normalize_q, nullptr, D_host, I_host);
}

// ------------------------------------------------------------------ group labels and grouped search
namespace {
// What the set and get entry points of a column share.  The arguments (`fn`, `arg`: the entry point and its host
// array in error strings); caller holds mu
int column_check(const char* fn, const char* arg, int64_t row0, int64_t n, int64_t ntotal, const void* host) {
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ntotal - row0, "%s: rows [%lld, %lld + %lld) outside [0, %lld)", fn,
                (long long)row0, (long long)row0, (long long)n, (long long)ntotal);
    CSS_REQUIRE(n == 0 || host, "%s: %s is NULL", fn, arg);
    return CSS_OK;
}
// The column ready for a set call's copies on the index's stream.  Rows appended on another stream write their default
// there: they must have landed before values go over them.  The first values of this index: the column, every row at
// the default.  Caller holds mu exclusively and the device
int column_for_write(css_index* ix, RowColumn* col) {
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(ix->stream, ix->ingest_ev, 0));
    return col->words.p ? CSS_OK : column_alloc(ix, *col, ix->cap, &col->words);
}
// Rows [row0, row0 + n) of the column to the host; a column that was never set answers its default
int column_get(css_index* ix, const RowColumn& col, const char* fn, const char* arg, int64_t row0, int64_t n, void* out_host) {
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    const int rc = column_check(fn, arg, row0, n, ix->ntotal, out_host);
    if (rc != CSS_OK || n == 0) return rc;
    if (!col.words.p) {
        memset(out_host, col.fill, (size_t)n * sizeof(int32_t));
        return CSS_OK;
    }
    DeviceGuard g(ix->device);
    if (ix->ingest_pending) CSS_HIP_TRY(hipEventSynchronize(ix->ingest_ev));
    CSS_HIP_TRY(hipMemcpy(out_host, col.words.p + row0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CSS_OK;
}
}  // namespace

int css_index_set_groups(css_index* ix, int64_t row0, int64_t n, const int32_t* labels_host) {
    CSS_REQUIRE(ix, "css_index_set_groups: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = column_check("css_index_set_groups", "labels", row0, n, ix->ntotal, labels_host);
    if (rc != CSS_OK || n == 0) return rc;
    DeviceGuard g(ix->device);
    if ((rc = column_for_write(ix, &ix->labels)) != CSS_OK) return rc;
    // negative labels are stored as -1: through a bounded host buffer
    const int64_t chunk = 1ll << 20;
    std::vector<int32_t> buf;
    try {
        buf.resize((size_t)std::min(n, chunk));
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_set_groups: out of host memory");
        return CSS_ERR_OOM;
    }
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        for (int64_t i = 0; i < m; ++i) buf[(size_t)i] = std::max<int32_t>(labels_host[r0 + i], -1);
        CSS_HIP_TRY(hipMemcpyAsync(ix->labels.words.p + row0 + r0, buf.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice,
                                   ix->stream));
        CSS_HIP_TRY(hipStreamSynchronize(ix->stream));   // (buf is written again)
    }
    return CSS_OK;
}

int css_index_get_groups(css_index* ix, int64_t row0, int64_t n, int32_t* labels_out_host) {
    CSS_REQUIRE(ix, "css_index_get_groups: NULL index");
    return column_get(ix, ix->labels, "css_index_get_groups", "labels_out", row0, n, labels_out_host);
}

// ------------------------------------------------------------------ attribute columns and css_index_where (css_where.h)
#define CSS_REQUIRE_SLOT(fn, slot) \
    CSS_REQUIRE((slot) >= 0 && (slot) < CSS_MAX_ATTRS, "%s: attribute slot %d outside [0, %d)", fn, (int)(slot), CSS_MAX_ATTRS)

int css_index_set_attr(css_index* ix, int slot, int type, int64_t row0, int64_t n, const void* values_host) {
    CSS_REQUIRE(ix, "css_index_set_attr: NULL index");
    CSS_REQUIRE_SLOT("css_index_set_attr", slot);
    CSS_REQUIRE(type == CSS_ATTR_I32 || type == CSS_ATTR_F32, "css_index_set_attr: type=%d is neither CSS_ATTR_I32 nor CSS_ATTR_F32", type);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    AttrColumn& col = ix->attrs[slot];
    CSS_REQUIRE(col.type < 0 || col.type == type, "css_index_set_attr: attribute slot %d holds %s values, not %s", slot,
                col.type == CSS_ATTR_I32 ? "int32" : "float32", type == CSS_ATTR_I32 ? "int32" : "float32");
    int rc = column_check("css_index_set_attr", "values", row0, n, ix->ntotal, values_host);
    if (rc != CSS_OK || n == 0) return rc;   // (no row, no type: a typed slot always has its column)
    DeviceGuard g(ix->device);
    if ((rc = column_for_write(ix, &col)) != CSS_OK) return rc;
    col.type = type;
    CSS_HIP_TRY(hipMemcpyAsync(col.words.p + row0, values_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ix->stream));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));   // (the caller's array is free again)
    return CSS_OK;
}

int css_index_get_attr(css_index* ix, int slot, int64_t row0, int64_t n, void* out_host) {
    CSS_REQUIRE(ix, "css_index_get_attr: NULL index");
    CSS_REQUIRE_SLOT("css_index_get_attr", slot);
    return column_get(ix, ix->attrs[slot], "css_index_get_attr", "out", row0, n, out_host);
}

int css_index_attr_type(css_index* ix, int slot, int* type) {
    CSS_REQUIRE(ix && type, "css_index_attr_type: NULL argument");
    CSS_REQUIRE_SLOT("css_index_attr_type", slot);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    *type = ix->attrs[slot].type;
    return CSS_OK;
}

int css_index_drop_attr(css_index* ix, int slot) {
    CSS_REQUIRE(ix, "css_index_drop_attr: NULL index");
    CSS_REQUIRE_SLOT("css_index_drop_attr", slot);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    AttrColumn& col = ix->attrs[slot];
    if (!col.words.p) return CSS_OK;
    DeviceGuard g(ix->device);
    // rows appended on another stream still write their default into the column
    if (ix->ingest_pending) CSS_HIP_TRY(hipEventSynchronize(ix->ingest_ev));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    col.type = -1;
    CSS_HIP_TRY(col.words.drop());
    return CSS_OK;
}

namespace {
// The clauses of a call checked against the slots and turned into what k_where reads; nothing is enqueued.  Caller
// holds mu (shared is enough: set and drop take it exclusively)
int where_args_of(css_index* ix, const css_clause* clauses, int nclauses, int64_t table_words, WhereArgs* out) {
    WhereArgs& a = *out;
    a.n = nclauses;
    for (int c = 0; c < nclauses; ++c) {
        const css_clause& cl = clauses[c];
        CSS_REQUIRE(cl.slot >= 0 && cl.slot < CSS_MAX_ATTRS, "css_index_where: clause %d: attribute slot %d outside [0, %d)", c,
                    (int)cl.slot, CSS_MAX_ATTRS);
        const AttrColumn& col = ix->attrs[cl.slot];
        CSS_REQUIRE(col.type >= 0 && col.words.p, "css_index_where: clause %d: attribute slot %d was never set", c, (int)cl.slot);
        CSS_REQUIRE(cl.op >= CSS_WHERE_EQ && cl.op <= CSS_WHERE_NOT_IN, "css_index_where: clause %d: unknown op %d", c, (int)cl.op);
        const bool f32 = col.type == CSS_ATTR_F32, in = cl.op >= CSS_WHERE_IN;
        CSS_REQUIRE(!(f32 && in), "css_index_where: clause %d: IN / NOT_IN on attribute slot %d, which holds float32 values", c,
                    (int)cl.slot);
        a.col[c] = col.as<const uint32_t>();
        a.key[c] = a.toff[c] = a.tbits[c] = 0u;
        int op = cl.op;
        if (in) {
            CSS_REQUIRE(cl.table_bits >= 0 && cl.table_bits <= CSS_MAX_TABLE_BITS, "css_index_where: clause %d: table_bits=%lld outside [0, %d]",
                        c, (long long)cl.table_bits, CSS_MAX_TABLE_BITS);
            CSS_REQUIRE(cl.table_off >= 0 && cl.table_off <= table_words && (cl.table_bits + 31) / 32 <= table_words - cl.table_off,
                        "css_index_where: clause %d: the table of %lld bits at word %lld does not lie inside the %lld table words", c,
                        (long long)cl.table_bits, (long long)cl.table_off, (long long)table_words);
            a.toff[c] = (uint32_t)cl.table_off;
            a.tbits[c] = (uint32_t)cl.table_bits;
        } else if (f32) {
            const uint32_t b = (uint32_t)cl.value;
            if (where_is_nan(b)) op = cl.op == CSS_WHERE_NE ? kWhereAlways : kWhereNever;
            a.key[c] = where_key_f32(b);
        } else {
            a.key[c] = where_key_i32((uint32_t)cl.value);
        }
        a.kind[c] = (uint32_t)op | (f32 ? 0x100u : 0u);
    }
    return CSS_OK;
}

// nrows > 0 rows inside the caller's host frame: tables and allow bitmap up, k_where, [count | bits] back.  Everything
// has finished on the index's own stream when this returns CSS_OK.
int where_locked(css_index* ix, HostCall& hc, const WhereArgs& a, const uint32_t* tables_host, int64_t table_words,
                 const uint32_t* allow_bits_host, uint32_t* bits_out_host, int64_t* count_out) {
    const hipStream_t st = ix->stream;
    const int64_t n = hc.rows.n, nwords = (n + 31) / 32, tiles = (n + kWhereTileRows - 1) / kWhereTileRows;
    int rc;
    WsTurn turn(ix, st);   // mask_ws, where_tab and where_out are shared workspaces
    if (turn.rc != CSS_OK) return turn.rc;
    if (table_words > 0) {
        if ((rc = hc.upload(allow_bits_host, ix->where_tab, tables_host, (size_t)table_words)) != CSS_OK) return rc;
    } else {
        hc.enqueued = true;
        if ((rc = upload_allow_bits(ix, allow_bits_host, &hc.rows)) != CSS_OK) return rc;
    }
    if ((rc = ix->where_out.grow((size_t)nwords + 2)) != CSS_OK) return rc;
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    unsigned long long* count = reinterpret_cast<unsigned long long*>(ix->where_out.p);
    uint32_t* bits = ix->where_out.p + 2;
    CSS_HIP_TRY(hipMemsetAsync(count, 0, sizeof(unsigned long long), st));
    // a block takes tiles in turn: enough blocks to fill the CUs, few enough that the LDS copy of the tables is rare
    const unsigned blocks = (unsigned)std::min<int64_t>(tiles, (int64_t)ix->num_cus * 8);
    const bool lds = table_words <= kWhereLdsWords;
    {
        ProfScope ps("where", st);
        if (lds)
            hipLaunchKernelGGL(k_where<true>, dim3(blocks), dim3(256), (size_t)table_words * sizeof(uint32_t), st, a, (const uint32_t*)ix->where_tab.p, (int)table_words,
                               hc.rows.mask, n, tiles, bits, count);
        else
            hipLaunchKernelGGL(k_where<false>, dim3(blocks), dim3(256), 0, st, a, (const uint32_t*)ix->where_tab.p, (int)table_words,
                               hc.rows.mask, n, tiles, bits, count);
        CSS_LAUNCH_CHECK();
    }
    const size_t bytes = ((size_t)nwords + 2) * sizeof(uint32_t);
    unsigned long long cnt = 0;
    if (ix->h_stage != nullptr && css_index::fits_host_stage(bytes)) {   // one copy, one wait (as read_ints)
        char* back = ix->h_stage + css_index::kHostStage;
        CSS_HIP_TRY(hipMemcpyAsync(back, ix->where_out.p, bytes, hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipStreamSynchronize(st));
        memcpy(&cnt, back, sizeof(cnt));
        memcpy(bits_out_host, back + 2 * sizeof(uint32_t), (size_t)nwords * sizeof(uint32_t));
    } else {
        CSS_HIP_TRY(hipMemcpyAsync(bits_out_host, bits, (size_t)nwords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipMemcpyAsync(&cnt, count, sizeof(cnt), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipStreamSynchronize(st));
    }
    *count_out = (int64_t)cnt;
    return CSS_OK;
}
}  // namespace

int css_index_where(css_index* ix, const css_clause* clauses, int nclauses, const uint32_t* tables_host, int64_t table_words,
                    const uint32_t* allow_bits_host, uint32_t* bits_out_host, int64_t* count_out) {
    CSS_REQUIRE(ix, "css_index_where: NULL index");
    CSS_REQUIRE(nclauses >= 0 && nclauses <= CSS_MAX_CLAUSES, "css_index_where: nclauses=%d outside [0, %d]", nclauses, CSS_MAX_CLAUSES);
    CSS_REQUIRE(nclauses == 0 || clauses, "css_index_where: clauses is NULL");
    CSS_REQUIRE(table_words >= 0 && table_words <= (int64_t)CSS_MAX_CLAUSES * (CSS_MAX_TABLE_BITS / 32),
                "css_index_where: table_words=%lld out of range", (long long)table_words);
    CSS_REQUIRE(table_words == 0 || tables_host, "css_index_where: tables is NULL");
    CSS_REQUIRE(count_out, "css_index_where: count_out is NULL");
    HostCall hc(ix, nullptr, false);
    WhereArgs a;
    const int rc = where_args_of(ix, clauses, nclauses, table_words, &a);
    if (rc != CSS_OK) return rc;
    *count_out = 0;
    if (hc.rows.n == 0) return CSS_OK;
    CSS_REQUIRE(bits_out_host, "css_index_where: bits_out is NULL");
    return hc.wait_if_failed(where_locked(ix, hc, a, tables_host, table_words, allow_bits_host, bits_out_host, count_out));
}

namespace {
// n ints from the device, through the pinned staging where it is there and large enough; waits for the stream
int read_ints(css_index* ix, const int* dev, size_t n, int* host) {
    const size_t bytes = n * sizeof(int);
    if (ix->h_stage != nullptr && css_index::fits_host_stage(bytes)) {
        char* back = ix->h_stage + css_index::kHostStage;
        CSS_HIP_TRY(hipMemcpyAsync(back, dev, bytes, hipMemcpyDeviceToHost, ix->stream));
        CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
        memcpy(host, back, bytes);
        return CSS_OK;
    }
    CSS_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ix->stream));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    return CSS_OK;
}

int launch_collapse(css_index* ix, const Rows& rows, int64_t q0, int64_t nqp, int kk, int k, float* Dg, int64_t* Ig,
                    int32_t* Lg, hipStream_t st) {
    hipLaunchKernelGGL(k_collapse_groups, dim3((unsigned)((nqp + 3) / 4)), dim3(256), 0, st, (const float*)ix->grp_d.p,
                       (const int64_t*)ix->grp_i.p, rows.labels, rows.id_base, q0, nqp, kk, k,
                       pad_score(ix), Dg, Ig, Lg, ix->grp_state.p);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// The passes of css_index_search_grouped over labelled rows (rows.labels set, rows.n > 0), on the index's own stream;
// Dg / Ig / Lg: device [nq, k].  Pass 1 serves the whole batch: the ordinary search for kk rows (the smaller list class
// of {32, 128} that holds 2k, else 128), one collapse launch, ONE readback of every query's [group count | exhausted].
// A query that has neither k groups nor a padded pass goes on alone, as the k > 128 path walks queries: its exclusion
// bitmap starts as the caller's bitmap and loses, in front of every pass, all rows of the groups found so far
// (k_mask_drop_groups; returned ungrouped rows one by one, k_mask_clear), so every pass of 128 rows brings at least one
// new group and a query takes at most k passes.  Scores of different passes may come from different summation orders:
// a query that took several passes is sorted once more (k_sort_rows), and its labels are gathered again behind that.
// Waits for the device (the pass count depends on the data).  Caller holds ws_mu and a shared lock on mu.
int search_grouped_passes(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, int normalize_q, float* Dg,
                          int64_t* Ig, int32_t* Lg) {
    const hipStream_t st = ix->stream;
    WsTurn turn(ix, st);   // excl_ws and the grp_* buffers are shared workspaces
    if (turn.rc != CSS_OK) return turn.rc;
    int rc;
    const int kk1 = 2 * k <= 32 ? 32 : CSS_KERNEL_MAX_K;
    if ((rc = ix->grp_d.grow((size_t)nq * kk1 + CSS_KERNEL_MAX_K)) != CSS_OK) return rc;
    if ((rc = ix->grp_i.grow((size_t)nq * kk1 + CSS_KERNEL_MAX_K)) != CSS_OK) return rc;
    if ((rc = ix->grp_state.grow((size_t)nq * 2)) != CSS_OK) return rc;   // [count, exhausted] per query
    CSS_HIP_TRY(hipMemsetAsync(ix->grp_state.p, 0, (size_t)nq * 2 * sizeof(int), st));
    if ((rc = search_any_k(ix, rows, q_dev, nq, kk1, normalize_q, ix->grp_d.p, ix->grp_i.p, st)) != CSS_OK) return rc;
    if ((rc = launch_collapse(ix, rows, 0, nq, kk1, k, Dg, Ig, Lg, st)) != CSS_OK) return rc;
    ix->last_group_passes = 1;
    std::vector<int> state((size_t)nq * 2);
    if ((rc = read_ints(ix, ix->grp_state.p, state.size(), state.data())) != CSS_OK) return rc;
    const int64_t words = (rows.n + 31) / 32;
    const unsigned drop_grid = (unsigned)std::min<int64_t>((rows.n + 255) / 256, (int64_t)ix->num_cus * 8);
    for (int64_t q = 0; q < nq; ++q) {
        if (state[2 * q] >= k || state[2 * q + 1]) continue;
        if ((rc = ix->excl_ws.grow((size_t)words)) != CSS_OK) return rc;
        Rows pass = rows;   // the same rows under the exclusion bitmap
        pass.mask = ix->excl_ws.p;
        hipLaunchKernelGGL(k_mask_init, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, ix->excl_ws.p, rows.mask, words);
        CSS_LAUNCH_CHECK();
        int qs[2] = {state[2 * q], 0};
        for (int p = 0; p < k && qs[0] < k && !qs[1]; ++p) {
            {
                ProfScope ps("knn_mask_drop_groups", st);
                hipLaunchKernelGGL(k_mask_drop_groups, dim3(drop_grid), dim3(256), 0, st, ix->excl_ws.p, rows.labels, rows.n,
                                   (const int32_t*)(Lg + (size_t)q * k), (const int*)(ix->grp_state.p + 2 * q));
                CSS_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL(k_mask_clear, dim3(1), dim3(CSS_KERNEL_MAX_K), 0, st, ix->excl_ws.p,
                               (const int64_t*)(Ig + (size_t)q * k), k, rows.id_base);
            CSS_LAUNCH_CHECK();
            if ((rc = search_dev_locked(ix, pass, q_dev + (size_t)q * ix->dim, 1, CSS_KERNEL_MAX_K, normalize_q, ix->grp_d.p,
                                        ix->grp_i.p, st)) != CSS_OK) return rc;
            if ((rc = launch_collapse(ix, rows, q, 1, CSS_KERNEL_MAX_K, k, Dg, Ig, Lg, st)) != CSS_OK) return rc;
            ++ix->last_group_passes;
            if ((rc = read_ints(ix, ix->grp_state.p + 2 * q, 2, qs)) != CSS_OK) return rc;
        }
        float* Dq = Dg + (size_t)q * k;
        int64_t* Iq = Ig + (size_t)q * k;
        if ((rc = launch_sort_rows(ix, Dq, Iq, 1, k, st)) != CSS_OK) return rc;
        hipLaunchKernelGGL(k_gather_labels, dim3(1), dim3(CSS_KERNEL_MAX_K), 0, st, (const int64_t*)Iq, rows.labels, rows.id_base,
                           (int64_t)k, Lg + (size_t)q * k);
        CSS_LAUNCH_CHECK();
    }
    return CSS_OK;
}
}  // namespace

int css_index_search_grouped(css_index* ix, const float* q_host, int64_t nq, int k, int normalize_q,
                             const uint32_t* allow_bits_host, float* D_host, int64_t* I_host, int32_t* G_host) {
    CSS_REQUIRE(ix, "css_index_search_grouped: NULL index");
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search_grouped: nq=%lld out of range", (long long)nq);
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "css_index_search_grouped: k=%d outside [1, %d]", k, CSS_KERNEL_MAX_K);
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(q_host && D_host && I_host, "css_index_search_grouped: NULL buffer");
    HostCall hc(ix);
    const size_t n = (size_t)nq * k;
    int rc = hc.upload(allow_bits_host, ix->q_raw, q_host, (size_t)nq * ix->dim, n, &ix->grp_l);
    // no labels (or no rows): every row is a group of its own, and the answer is the masked search's, G = -1
    const bool labelled = hc.rows.labels != nullptr && hc.rows.n > 0;
    if (rc == CSS_OK && labelled) {
        rc = search_grouped_passes(ix, hc.rows, ix->q_raw.p, nq, k, normalize_q, hc.d_out, hc.i_out, hc.g_out);
    } else if (rc == CSS_OK) {
        rc = search_any_k(ix, hc.rows, ix->q_raw.p, nq, k, normalize_q, hc.d_out, hc.i_out, ix->stream);
        ix->last_group_passes = 1;
        if (rc == CSS_OK && G_host) std::fill(G_host, G_host + n, (int32_t)-1);
    }
    return hc.finish(rc, D_host, I_host, labelled ? G_host : nullptr);
}

int css_index_last_group_passes(css_index* ix, int64_t* n) {
    CSS_REQUIRE(ix && n, "css_index_last_group_passes: NULL argument");
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    *n = ix->last_group_passes;
    return CSS_OK;
}

// ------------------------------------------------------------------ diversified search (MMR over a pool of the best rows)
namespace {
// lam in [0, 1], fetch 0 (automatic: the two list classes of the grouped search) or in [1, 128], 1 <= k <= fetch
int check_diverse_args(const char* fn, int k, int* fetch, float lam) {
    CSS_REQUIRE(lam >= 0.f && lam <= 1.f, "%s: lam=%g outside [0, 1]", fn, (double)lam);   // (a NaN fails both)
    CSS_REQUIRE(*fetch >= 0 && *fetch <= CSS_KERNEL_MAX_K, "%s: fetch=%d outside [0, %d] (0: automatic)", fn, *fetch,
                CSS_KERNEL_MAX_K);
    if (*fetch == 0) *fetch = (k <= 8) ? 32 : CSS_KERNEL_MAX_K;   // 4k <= 32
    CSS_REQUIRE(k >= 1 && k <= *fetch, "%s: k=%d outside [1, fetch=%d]", fn, k, *fetch);
    return CSS_OK;
}

// The ordinary search for the pool (search_any_k: every mode, shadow policy and mask as css_index_search_masked_dev
// has them) into the owned pool lists, and the selection behind it.  Everything is enqueued on `st`; nothing waits
// for the device.  Caller holds ws_mu and a shared lock on mu.
int search_diverse_enqueue(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, int fetch, float lam,
                           int normalize_q, float* D_dev, int64_t* I_dev, hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);   // (until the end: the selection reads the pool lists)
    if (turn.rc != CSS_OK) return turn.rc;
    // rows appended on another stream must have landed (an empty pool search does not wait for them itself)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->div_d.grow((size_t)nq * fetch)) != CSS_OK) return rc;
    if ((rc = ix->div_i.grow((size_t)nq * fetch)) != CSS_OK) return rc;
    if ((rc = search_any_k(ix, rows, q_dev, nq, fetch, normalize_q, ix->div_d.p, ix->div_i.p, st)) != CSS_OK) return rc;
    ProfScope ps("knn_mmr_select", st);
    if (ix->metric == CSS_METRIC_IP)
        hipLaunchKernelGGL(k_mmr_select<CSS_METRIC_IP>, dim3((unsigned)nq), dim3(256), 0, st, (const float*)ix->div_d.p,
                           (const int64_t*)ix->div_i.p, rows.xb, rows.n, rows.id_base, ix->dim, ix->dpad, fetch, k, lam,
                           pad_score(ix), D_dev, I_dev);
    else
        hipLaunchKernelGGL(k_mmr_select<CSS_METRIC_L2>, dim3((unsigned)nq), dim3(256), 0, st, (const float*)ix->div_d.p,
                           (const int64_t*)ix->div_i.p, rows.xb, rows.n, rows.id_base, ix->dim, ix->dpad, fetch, k, lam,
                           pad_score(ix), D_dev, I_dev);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}
}  // namespace

int css_index_search_diverse_dev(css_index* ix, const float* q_dev, int64_t nq, int k, int fetch, float lam, int normalize_q,
                                 const uint32_t* allow_bits_dev, float* D_dev, int64_t* I_dev, void* stream) {
    CSS_REQUIRE(ix, "css_index_search_diverse_dev: NULL index");
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search_diverse_dev: nq=%lld out of range", (long long)nq);
    int rc;
    if ((rc = check_diverse_args("css_index_search_diverse_dev", k, &fetch, lam)) != CSS_OK) return rc;
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(q_dev && D_dev && I_dev, "css_index_search_diverse_dev: NULL buffer");
    CallScope cs(ix, allow_bits_dev);
    return search_diverse_enqueue(ix, cs.rows, q_dev, nq, k, fetch, lam, normalize_q, D_dev, I_dev,
                                  (hipStream_t)stream);
}

int css_index_search_diverse(css_index* ix, const float* q_host, int64_t nq, int k, int fetch, float lam, int normalize_q,
                             const uint32_t* allow_bits_host, float* D_host, int64_t* I_host) {
    CSS_REQUIRE(ix, "css_index_search_diverse: NULL index");
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search_diverse: nq=%lld out of range", (long long)nq);
    int rc;
    if ((rc = check_diverse_args("css_index_search_diverse", k, &fetch, lam)) != CSS_OK) return rc;
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(q_host && D_host && I_host, "css_index_search_diverse: NULL buffer");
    HostCall hc(ix);
    rc = hc.upload(allow_bits_host, ix->q_raw, q_host, (size_t)nq * ix->dim, (size_t)nq * k);
    if (rc == CSS_OK)
        rc = search_diverse_enqueue(ix, hc.rows, ix->q_raw.p, nq, k, fetch, lam, normalize_q, hc.d_out, hc.i_out, ix->stream);
    return hc.finish(rc, D_host, I_host);
}

namespace {
// The anchors' rows gathered as queries, the ordinary search (search_any_k: every mode, shadow policy, k and chunking
// as css_index_search_masked_dev has them) at k + 1 when the anchor is to go, and the compaction to k.  Everything is
// enqueued on `st`.  Caller holds ws_mu and a shared lock on mu.
int search_rows_enqueue(css_index* ix, const Rows& rows, const int64_t* ids_dev, int64_t nq, int k, int exclude_self,
                        float* D_dev, int64_t* I_dev, hipStream_t st) {
    const int kk = k + (exclude_self ? 1 : 0);
    int rc;
    WsTurn turn(ix, st);   // (until the end: whatever is launched uses the gathered rows)
    if (turn.rc != CSS_OK) return turn.rc;
    // rows appended on another stream must have landed
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->rowq.grow((size_t)nq * ix->dim)) != CSS_OK) return rc;
    if ((rc = ix->rowq_flag.grow((size_t)nq)) != CSS_OK) return rc;
    if ((rc = ix->rowq_d.grow((size_t)nq * kk)) != CSS_OK) return rc;
    if ((rc = ix->rowq_i.grow((size_t)nq * kk)) != CSS_OK) return rc;
    const dim3 grid((unsigned)((nq + 3) / 4));
    hipLaunchKernelGGL(k_gather_queries, grid, dim3(256), 0, st, rows.xb, ids_dev, ix->rowq.p, ix->rowq_flag.p, nq, rows.n,
                       rows.id_base, ix->dim, ix->dpad);
    CSS_LAUNCH_CHECK();
    if ((rc = search_any_k(ix, rows, ix->rowq.p, nq, kk, 0, ix->rowq_d.p, ix->rowq_i.p, st)) != CSS_OK) return rc;
    hipLaunchKernelGGL(k_drop_self, grid, dim3(256), 0, st, (const float*)ix->rowq_d.p, (const int64_t*)ix->rowq_i.p, ids_dev,
                       (const int*)ix->rowq_flag.p, nq, kk, k, exclude_self ? 1 : 0, pad_score(ix), D_dev, I_dev);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

int check_search_rows_k(int k, int exclude_self) {
    const int kmax = exclude_self ? CSS_MAX_K - 1 : CSS_MAX_K;
    CSS_REQUIRE(k >= 1 && k <= kmax, "css_index_search_rows: k=%d outside [1, %d]%s", k, kmax,
                exclude_self ? " (exclude_self searches for k + 1)" : "");
    return CSS_OK;
}
}  // namespace

int css_index_search_rows_dev(css_index* ix, const int64_t* ids_dev, int64_t nq, int k, int exclude_self,
                              const uint32_t* allow_bits_dev, float* D_dev, int64_t* I_dev, void* stream) {
    CSS_REQUIRE(ix, "css_index_search_rows_dev: NULL index");
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search_rows_dev: nq=%lld out of range", (long long)nq);
    int rc;
    if ((rc = check_search_rows_k(k, exclude_self)) != CSS_OK) return rc;
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(ids_dev && D_dev && I_dev, "css_index_search_rows_dev: NULL buffer");
    CallScope cs(ix, allow_bits_dev);
    return search_rows_enqueue(ix, cs.rows, ids_dev, nq, k, exclude_self, D_dev, I_dev, (hipStream_t)stream);
}

int css_index_search_rows(css_index* ix, const int64_t* ids_host, int64_t nq, int k, int exclude_self,
                          const uint32_t* allow_bits_host, float* D_host, int64_t* I_host) {
    CSS_REQUIRE(ix, "css_index_search_rows: NULL index");
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search_rows: nq=%lld out of range", (long long)nq);
    int rc;
    if ((rc = check_search_rows_k(k, exclude_self)) != CSS_OK) return rc;
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(ids_host && D_host && I_host, "css_index_search_rows: NULL buffer");
    HostCall hc(ix);
    const Rows& rows = hc.rows;   // (the host id range check comes before anything is enqueued)
    for (int64_t j = 0; j < nq; ++j)
        CSS_REQUIRE(ids_host[j] >= rows.id_base && ids_host[j] - rows.id_base < rows.n,
                    "css_index_search_rows: id %lld (query %lld) outside [%lld, %lld)", (long long)ids_host[j], (long long)j,
                    (long long)rows.id_base, (long long)(rows.id_base + rows.n));
    rc = hc.upload(allow_bits_host, ix->rowq_ids, ids_host, (size_t)nq, (size_t)nq * k);
    if (rc == CSS_OK) rc = search_rows_enqueue(ix, rows, ix->rowq_ids.p, nq, k, exclude_self, hc.d_out, hc.i_out, ix->stream);
    return hc.finish(rc, D_host, I_host);
}

// ------------------------------------------------------------------ per-row priors and prior-weighted search
int css_index_set_priors(css_index* ix, int64_t row0, int64_t n, const float* priors_host) {
    CSS_REQUIRE(ix, "css_index_set_priors: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    int rc = column_check("css_index_set_priors", "priors", row0, n, ix->ntotal, priors_host);
    if (rc != CSS_OK || n == 0) return rc;
    // every value is looked at before anything is written
    for (int64_t i = 0; i < n; ++i)
        CSS_REQUIRE(std::isfinite(priors_host[i]), "css_index_set_priors: the prior of row %lld is %s (priors are finite)",
                    (long long)(row0 + i), std::isnan(priors_host[i]) ? "NaN" : "infinite");
    DeviceGuard g(ix->device);
    if ((rc = column_for_write(ix, &ix->priors)) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemcpyAsync(ix->priors.as<float>() + row0, priors_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));   // (the copy reads the caller's memory)
    return CSS_OK;
}

int css_index_get_priors(css_index* ix, int64_t row0, int64_t n, float* priors_out_host) {
    CSS_REQUIRE(ix, "css_index_get_priors: NULL index");
    return column_get(ix, ix->priors, "css_index_get_priors", "priors_out", row0, n, priors_out_host);
}

namespace {
// Query prep, the prior sweeps (sg.nq_sweep queries each, at most 16), and the raw scores of the returned rows behind
// them.  Everything is enqueued on `st`; nothing waits for the device.  Caller holds ws_mu and a shared lock on mu.
int search_prior_enqueue(css_index* ix, const Rows& rows, const float* q_dev, int64_t nq, int k, float weight, int normalize_q,
                         float* D_dev, int64_t* I_dev, float* S_dev, hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    // rows appended on another stream must have landed
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->qpad.grow((size_t)(nq + 256) * ix->dpad)) != CSS_OK) return rc;
    if ((rc = ix->qnorm2.grow((size_t)nq + 256)) != CSS_OK) return rc;
    if ((rc = ix->gthr.grow((size_t)nq + 256)) != CSS_OK) return rc;
    if ((rc = prep_queries(ix, q_dev, nq, normalize_q, nullptr, st)) != CSS_OK) return rc;
    const int64_t n = nq * k;
    if (rows.n == 0) {
        hipLaunchKernelGGL(k_fill_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D_dev, I_dev, n, pad_score(ix));
        CSS_LAUNCH_CHECK();
    } else {
        CSS_REQUIRE(rows.n < 0xFFFFFFFFll, "css_index_search_prior: %lld rows exceed the 32-bit row numbers of the lists",
                    (long long)rows.n);
        SweepGeom sg;
        if ((rc = make_sweep_geom(ix, rows, k, &sg)) != CSS_OK) return rc;
        if ((rc = grow_part(ix, (size_t)sg.nq_sweep * sg.G * k)) != CSS_OK) return rc;
        for (int64_t q0 = 0; q0 < nq; q0 += sg.nq_sweep) {
            const int nqc = (int)std::min<int64_t>(sg.nq_sweep, nq - q0);
            if ((rc = search_chunk_prior(ix, rows, (int)q0, nqc, k, weight, sg, D_dev, I_dev, st)) != CSS_OK) return rc;
        }
    }
    // (an empty index: every slot is padded and no row is read)
    ProfScope ps("knn_prior_scores", st);
    const dim3 grid((unsigned)((n + 15) / 16));
    if (ix->metric == CSS_METRIC_IP)
        hipLaunchKernelGGL(k_prior_scores<CSS_METRIC_IP>, grid, dim3(256), 0, st, (const float4*)rows.xb, (const float*)ix->qpad.p,
                           (const int64_t*)I_dev, n, k, ix->dpad / 64, rows.id_base, pad_score(ix), S_dev);
    else
        hipLaunchKernelGGL(k_prior_scores<CSS_METRIC_L2>, grid, dim3(256), 0, st, (const float4*)rows.xb, (const float*)ix->qpad.p,
                           (const int64_t*)I_dev, n, k, ix->dpad / 64, rows.id_base, pad_score(ix), S_dev);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}
}  // namespace

int css_index_search_prior(css_index* ix, const float* q_host, int64_t nq, int k, float weight, int normalize_q,
                           const uint32_t* allow_bits_host, float* D_host, int64_t* I_host, float* S_host) {
    CSS_REQUIRE(ix, "css_index_search_prior: NULL index");
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_search_prior: nq=%lld out of range", (long long)nq);
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "css_index_search_prior: k=%d outside [1, %d]", k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(std::isfinite(weight), "css_index_search_prior: weight is %s (it must be finite)",
                std::isnan(weight) ? "NaN" : "infinite");
    if (nq == 0) return CSS_OK;
    CSS_REQUIRE(q_host && D_host && I_host, "css_index_search_prior: NULL buffer");
    HostCall hc(ix);
    int rc = hc.upload(allow_bits_host, ix->q_raw, q_host, (size_t)nq * ix->dim, (size_t)nq * k, &ix->pri_s);
    if (rc == CSS_OK)
        rc = search_prior_enqueue(ix, hc.rows, ix->q_raw.p, nq, k, weight, normalize_q, hc.d_out, hc.i_out,
                                  reinterpret_cast<float*>(hc.g_out), ix->stream);
    return hc.finish(rc, D_host, I_host, reinterpret_cast<int32_t*>(S_host));   // (S rides in the 4-byte column)
}

// ------------------------------------------------------------------ search by examples
namespace {
// What css_index_search_examples uploads in ONE copy (floats of q_raw): the id examples, the excluded local rows, and
// the raw example table [m][dim] in table order -- positive vectors, positive ids, negative vectors, negative ids --
// with the rows of the id examples left for k_gather_queries to fill.
constexpr size_t kExIdsAt = 0;                                   // int64[kMaxExamples]
constexpr size_t kExExclAt = kMaxExamples * 2;                   // uint32[kMaxExamples]
constexpr size_t kExTableAt = kMaxExamples * 3;                  // float[m][dim]; 192 bytes in: 16-byte aligned

struct ExampleCounts {
    int vec_pos, vec_neg, id_pos, id_neg;
    int npos() const { return vec_pos + id_pos; }
    int m() const { return vec_pos + id_pos + vec_neg + id_neg; }
};

// Example table, sweep, merge, and S behind them.  in_dev: the upload described above.  Everything is enqueued on
// `st`; nothing waits for the device.  Caller holds ws_mu and a shared lock on mu.
int search_examples_enqueue(css_index* ix, const Rows& rows, const float* in_dev, const ExampleCounts& c, int k, float gamma,
                            int normalize_vec, int nexcl, float* D_dev, int64_t* I_dev, float* S_dev, hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    // rows appended on another stream must have landed
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->qpad.grow((size_t)(kMaxExamples + 256) * ix->dpad)) != CSS_OK) return rc;
    if ((rc = ix->qnorm2.grow((size_t)kMaxExamples + 256)) != CSS_OK) return rc;
    if ((rc = ix->gthr.grow((size_t)kMaxExamples + 256)) != CSS_OK) return rc;
    if ((rc = ix->rowq_flag.grow((size_t)kMaxExamples)) != CSS_OK) return rc;
    const int64_t* ids_dev = reinterpret_cast<const int64_t*>(in_dev + kExIdsAt);
    float* table = const_cast<float*>(in_dev) + kExTableAt;
    // the four segments of the table: rows, whether they are stored rows, and their first id in ids_dev
    const struct { int n; bool ids; int id0; } seg[4] = {
        {c.vec_pos, false, 0}, {c.id_pos, true, 0}, {c.vec_neg, false, 0}, {c.id_neg, true, c.id_pos}};
    // stored rows as they lie in HBM (the host has checked every id: no flag is read)
    for (int s = 0, r0 = 0; s < 4; r0 += seg[s++].n)
        if (seg[s].ids && seg[s].n > 0) {
            hipLaunchKernelGGL(k_gather_queries, dim3((unsigned)((seg[s].n + 3) / 4)), dim3(256), 0, st, rows.xb,
                               ids_dev + seg[s].id0, table + (size_t)r0 * ix->dim, ix->rowq_flag.p, (int64_t)seg[s].n, rows.n,
                               rows.id_base, ix->dim, ix->dpad);
            CSS_LAUNCH_CHECK();
        }
    // prep_queries over runs of neighbouring segments that are normalised alike (stored rows never are)
    for (int s = 0, r0 = 0; s < 4;) {
        const int flag = !seg[s].ids && normalize_vec ? 1 : 0;
        int n = 0, e = s;
        for (; e < 4 && (seg[e].n == 0 || (!seg[e].ids && normalize_vec ? 1 : 0) == flag); ++e) n += seg[e].n;
        if (n > 0 && (rc = prep_queries(ix, table + (size_t)r0 * ix->dim, n, flag, nullptr, st, r0)) != CSS_OK) return rc;
        r0 += n;
        s = e;
    }
    if (rows.n == 0) {
        hipLaunchKernelGGL(k_fill_pad, dim3(1), dim3(256), 0, st, D_dev, I_dev, (int64_t)k, pad_score(ix));
        CSS_LAUNCH_CHECK();
    } else {
        SweepGeom sg;
        sweep_grid(ix, rows, &sg.G, &sg.gpb);
        sg.nq_sweep = 1;   // (one list)
        if ((rc = grow_part(ix, (size_t)sg.G * k)) != CSS_OK) return rc;
        const ExampleArgs ea{c.npos(), c.m(), gamma, reinterpret_cast<const uint32_t*>(in_dev + kExExclAt), nexcl};
        if ((rc = search_examples_sweep(ix, rows, k, ea, sg, D_dev, I_dev, st)) != CSS_OK) return rc;
    }
    if (!S_dev) return CSS_OK;
    // (an empty index: every slot is padded and no row is read)
    ProfScope ps("knn_example_scores", st);
    if (ix->metric == CSS_METRIC_IP)
        hipLaunchKernelGGL(k_example_scores<CSS_METRIC_IP>, dim3(k), dim3(256), 0, st, (const float4*)rows.xb,
                           (const float*)ix->qpad.p, (const int64_t*)I_dev, c.npos(), ix->dpad / 64, rows.id_base, pad_score(ix), S_dev);
    else
        hipLaunchKernelGGL(k_example_scores<CSS_METRIC_L2>, dim3(k), dim3(256), 0, st, (const float4*)rows.xb,
                           (const float*)ix->qpad.p, (const int64_t*)I_dev, c.npos(), ix->dpad / 64, rows.id_base, pad_score(ix), S_dev);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}
}  // namespace

int css_index_search_examples(css_index* ix, const float* vec_host, int nvec_pos, int nvec_neg, const int64_t* ids_host,
                              int nid_pos, int nid_neg, int k, float gamma, int normalize_vec, int exclude_ids,
                              const uint32_t* allow_bits_host, float* D_host, int64_t* I_host, float* S_host) {
    CSS_REQUIRE(ix, "css_index_search_examples: NULL index");
    CSS_REQUIRE(nvec_pos >= 0 && nvec_neg >= 0 && nid_pos >= 0 && nid_neg >= 0,
                "css_index_search_examples: negative example count (%d, %d, %d, %d)", nvec_pos, nvec_neg, nid_pos, nid_neg);
    CSS_REQUIRE(nvec_pos <= CSS_MAX_EXAMPLES && nvec_neg <= CSS_MAX_EXAMPLES && nid_pos <= CSS_MAX_EXAMPLES &&
                    nid_neg <= CSS_MAX_EXAMPLES && nvec_pos + nvec_neg + nid_pos + nid_neg <= CSS_MAX_EXAMPLES,
                "css_index_search_examples: more than %d examples (%d + %d vectors, %d + %d ids)", CSS_MAX_EXAMPLES, nvec_pos,
                nvec_neg, nid_pos, nid_neg);
    const ExampleCounts c{nvec_pos, nvec_neg, nid_pos, nid_neg};
    CSS_REQUIRE(c.npos() >= 1, "css_index_search_examples: no positive example");
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "css_index_search_examples: k=%d outside [1, %d]", k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, "css_index_search_examples: gamma is %s (it must be finite and >= 0)",
                std::isnan(gamma) ? "NaN" : std::isinf(gamma) ? "infinite" : "negative");
    const int nvec = nvec_pos + nvec_neg, nid = nid_pos + nid_neg;
    CSS_REQUIRE(D_host && I_host && (nvec == 0 || vec_host) && (nid == 0 || ids_host), "css_index_search_examples: NULL buffer");
    HostCall hc(ix);
    const Rows& rows = hc.rows;   // (every host check comes before anything is enqueued)
    for (int j = 0; j < nid; ++j)
        CSS_REQUIRE(ids_host[j] >= rows.id_base && ids_host[j] - rows.id_base < rows.n,
                    "css_index_search_examples: id %lld (%s example %d) outside [%lld, %lld)", (long long)ids_host[j],
                    j < nid_pos ? "positive" : "negative", j < nid_pos ? j : j - nid_pos, (long long)rows.id_base,
                    (long long)(rows.id_base + rows.n));
    CSS_REQUIRE(rows.n < 0xFFFFFFFFll, "css_index_search_examples: %lld rows exceed the 32-bit row numbers of the lists",
                (long long)rows.n);
    CSS_REQUIRE(examples_lds(examples_slots(c.m()), ix->dpad, k) <= 64 * 1024,
                "css_index_search_examples: %d examples of dim=%d exceed the sweep's example table (64 KiB with its list)", c.m(),
                ix->dim);
    // the ONE upload: ids, excluded local rows, the raw table with the vector examples in their places
    const size_t dim = (size_t)ix->dim;
    std::vector<float> in(kExTableAt + (size_t)c.m() * dim, 0.f);
    if (nid) memcpy(in.data() + kExIdsAt, ids_host, (size_t)nid * sizeof(int64_t));
    const int nexcl = exclude_ids ? nid : 0;
    for (int j = 0; j < nexcl; ++j) {
        const uint32_t r = (uint32_t)(ids_host[j] - rows.id_base);
        memcpy(in.data() + kExExclAt + j, &r, sizeof r);
    }
    if (nvec_pos) memcpy(in.data() + kExTableAt, vec_host, (size_t)nvec_pos * dim * sizeof(float));
    if (nvec_neg)
        memcpy(in.data() + kExTableAt + (size_t)c.npos() * dim, vec_host + (size_t)nvec_pos * dim, (size_t)nvec_neg * dim * sizeof(float));
    int rc = hc.upload(allow_bits_host, ix->q_raw, (const float*)in.data(), in.size(), (size_t)k, S_host ? &ix->ex_s : nullptr);
    if (rc == CSS_OK)
        rc = search_examples_enqueue(ix, rows, ix->q_raw.p, c, k, gamma, normalize_vec, nexcl, hc.d_out, hc.i_out,
                                     reinterpret_cast<float*>(hc.g_out), ix->stream);
    return hc.finish(rc, D_host, I_host, reinterpret_cast<int32_t*>(S_host));   // (S rides in the 4-byte column)
}

// ------------------------------------------------------------------ per-row term lists and hybrid search
namespace {
// `b` grown to `need` elements (at least doubled) with its first `keep` elements kept (an empty `b` has none to keep);
// the index's stream is drained before the old buffer goes
extern "C++" template <typename T>
int grow_keep(css_index* ix, DevBuf<T>& b, size_t keep, size_t need, const char* what) {
    if (need <= b.cap) return CSS_OK;
    DevBuf<T> nb;
    int rc;
    if ((rc = nb.grow_exact(std::max(need, b.cap * 2), what)) != CSS_OK) return rc;
    if (keep && b.p) CSS_HIP_TRY(hipMemcpyAsync(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, ix->stream));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    b.swap(nb);
    return CSS_OK;
}
}  // namespace

int css_index_set_terms(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host, const uint32_t* tokens_host) {
    CSS_REQUIRE(ix, "css_index_set_terms: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);   // (ws_pending)
    const int64_t T0 = ix->lex_rows;
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "css_index_set_terms: rows [%lld, %lld + %lld) outside [0, %lld)",
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(row0 <= T0, "css_index_set_terms: row0=%lld beyond the %lld rows that have lists (lists are append-only)",
                (long long)row0, (long long)T0);
    CSS_REQUIRE(n == 0 || offsets_host, "css_index_set_terms: offsets is NULL");
    // everything is looked at before anything is written
    if (n > 0) {
        CSS_REQUIRE(offsets_host[0] == 0, "css_index_set_terms: offsets start at %lld, not 0", (long long)offsets_host[0]);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t c = offsets_host[i + 1] - offsets_host[i];
            CSS_REQUIRE(c >= 0, "css_index_set_terms: offsets decrease at row %lld", (long long)(row0 + i));
            CSS_REQUIRE(c <= CSS_MAX_ROW_TOKENS, "css_index_set_terms: row %lld has %lld tokens (at most %d)", (long long)(row0 + i),
                        (long long)c, CSS_MAX_ROW_TOKENS);
        }
        CSS_REQUIRE(offsets_host[n] == 0 || tokens_host, "css_index_set_terms: tokens is NULL");
        for (int64_t i = 0; i < n; ++i)
            for (int64_t t = offsets_host[i]; t < offsets_host[i + 1]; ++t)
                CSS_REQUIRE(tokens_host[t] < CSS_TERM_SPACE, "css_index_set_terms: token %u of row %lld is outside [0, 2^24)",
                            tokens_host[t], (long long)(row0 + i));
    }
    if (n == 0 && row0 == T0) return CSS_OK;
    // each row sorted and counted on the host: term << 8 | min(tf, 255), ascending by term
    std::vector<uint32_t> ent, dl, tmp;
    std::vector<int64_t> off;
    const int64_t E0 = T0 > 0 ? ix->lex_off_h[(size_t)row0] : 0;
    try {
        ent.reserve(n > 0 ? (size_t)offsets_host[n] : 0);
        dl.resize((size_t)n);
        off.resize((size_t)n + 1);
        off[0] = E0;
        for (int64_t i = 0; i < n; ++i) {
            tmp.assign(tokens_host + offsets_host[i], tokens_host + offsets_host[i + 1]);
            std::sort(tmp.begin(), tmp.end());
            for (size_t a = 0; a < tmp.size();) {
                size_t e = a;
                while (e < tmp.size() && tmp[e] == tmp[a]) ++e;
                ent.push_back(tmp[a] << 8 | (uint32_t)std::min<size_t>(e - a, 255));
                a = e;
            }
            dl[(size_t)i] = (uint32_t)tmp.size();
            off[(size_t)i + 1] = E0 + (int64_t)ent.size();
        }
        ix->lex_off_h.reserve((size_t)(row0 + n) + 1);
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_set_terms: out of host memory");
        return CSS_ERR_OOM;
    }
    DeviceGuard g(ix->device);
    const hipStream_t st = ix->stream;
    // as css_index_set_groups; and a search on another stream may still read the lists that go or move
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if (ix->ws_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ws_ev, 0));
    int rc;
    if (!ix->lex_df.p) {   // first terms of this index: the statistics, all zero
        if ((rc = ix->lex_total.grow_exact(1, "hipMalloc(term statistics)")) != CSS_OK) return rc;
        if ((rc = ix->lex_df.grow_exact((size_t)CSS_TERM_SPACE, "hipMalloc(term statistics)")) != CSS_OK) return rc;
        CSS_HIP_TRY(hipMemsetAsync(ix->lex_df.p, 0, (size_t)CSS_TERM_SPACE * sizeof(uint32_t), st));
        CSS_HIP_TRY(hipMemsetAsync(ix->lex_total.p, 0, sizeof(unsigned long long), st));
        ix->lex_off_h.assign(1, 0);
    }
    if (row0 < T0) {   // the lists of rows >= row0 go, and leave the statistics
        const int64_t gone = ix->lex_off_h[(size_t)T0] - E0;
        if (gone > 0) {
            hipLaunchKernelGGL(k_lex_df_add, dim3(lex_grid(ix, gone)), dim3(256), 0, st, (const uint32_t*)ix->lex_ent.p + E0, gone,
                               ix->lex_df.p, 0xFFFFFFFFu);
            CSS_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_lex_len_add, dim3(lex_grid(ix, T0 - row0)), dim3(256), 0, st, (const uint32_t*)ix->lex_dl.p + row0,
                           T0 - row0, ix->lex_total.p, 1);
        CSS_LAUNCH_CHECK();
        ix->lex_off_h.resize((size_t)row0 + 1);
        ix->lex_rows = row0;
    }
    if (n > 0) {
        const size_t nE = ent.size();
        if ((rc = grow_keep(ix, ix->lex_ent, (size_t)E0, (size_t)E0 + std::max<size_t>(nE, 1), "hipMalloc(term lists)")) != CSS_OK) return rc;
        if ((rc = grow_keep(ix, ix->lex_dl, (size_t)row0, (size_t)(row0 + n), "hipMalloc(term lists)")) != CSS_OK) return rc;
        if ((rc = grow_keep(ix, ix->lex_off, (size_t)row0 + 1, (size_t)(row0 + n) + 1, "hipMalloc(term lists)")) != CSS_OK) return rc;
        if (nE) CSS_HIP_TRY(hipMemcpyAsync(ix->lex_ent.p + E0, ent.data(), nE * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        CSS_HIP_TRY(hipMemcpyAsync(ix->lex_dl.p + row0, dl.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        CSS_HIP_TRY(hipMemcpyAsync(ix->lex_off.p + row0, off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (nE) {
            hipLaunchKernelGGL(k_lex_df_add, dim3(lex_grid(ix, (int64_t)nE)), dim3(256), 0, st, (const uint32_t*)ix->lex_ent.p + E0,
                               (int64_t)nE, ix->lex_df.p, 1u);
            CSS_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_lex_len_add, dim3(lex_grid(ix, n)), dim3(256), 0, st, (const uint32_t*)ix->lex_dl.p + row0, n,
                           ix->lex_total.p, 0);
        CSS_LAUNCH_CHECK();
    }
    CSS_HIP_TRY(hipStreamSynchronize(st));   // (the copies read this call's vectors)
    ix->lex_off_h.insert(ix->lex_off_h.end(), off.begin() + 1, off.end());
    ix->lex_rows = row0 + n;
    return CSS_OK;
}

int css_index_get_terms(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out, uint32_t* entries_out, uint32_t* dl_out) {
    CSS_REQUIRE(ix, "css_index_get_terms: NULL index");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "css_index_get_terms: rows [%lld, %lld + %lld) outside [0, %lld)",
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(offsets_out, "css_index_get_terms: offsets_out is NULL");
    const int64_t T = ix->lex_rows;
    const int64_t a = std::min(row0, T), e = std::min(row0 + n, T);   // the rows of the range that have lists
    const int64_t E0 = T > 0 ? ix->lex_off_h[(size_t)a] : 0;
    for (int64_t i = 0; i <= n; ++i) offsets_out[i] = T > 0 ? ix->lex_off_h[(size_t)std::min(row0 + i, T)] - E0 : 0;
    if (dl_out) std::fill(dl_out, dl_out + n, 0u);
    if (e <= a) return CSS_OK;
    DeviceGuard g(ix->device);
    if (entries_out && offsets_out[n] > 0)
        CSS_HIP_TRY(hipMemcpy(entries_out, ix->lex_ent.p + E0, (size_t)offsets_out[n] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (dl_out) CSS_HIP_TRY(hipMemcpy(dl_out, ix->lex_dl.p + a, (size_t)(e - a) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CSS_OK;
}

int css_index_term_stats(css_index* ix, const uint32_t* terms_host, int m, int64_t* df_out, int64_t* ndocs_out,
                         int64_t* total_len_out) {
    CSS_REQUIRE(ix, "css_index_term_stats: NULL index");
    CSS_REQUIRE(m >= 0 && m <= (1 << 20), "css_index_term_stats: m=%d outside [0, 2^20]", m);
    CSS_REQUIRE(ndocs_out && total_len_out && (m == 0 || (terms_host && df_out)), "css_index_term_stats: NULL buffer");
    for (int j = 0; j < m; ++j)
        CSS_REQUIRE(terms_host[j] < CSS_TERM_SPACE, "css_index_term_stats: term %u (number %d) is outside [0, 2^24)", terms_host[j], j);
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    *ndocs_out = ix->ntotal;
    *total_len_out = 0;
    std::fill(df_out, df_out + m, (int64_t)0);
    if (!ix->lex_df.p) return CSS_OK;
    DeviceGuard g(ix->device);
    const hipStream_t st = ix->stream;
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if ((rc = ix->lex_ask.grow((size_t)m + 1)) != CSS_OK) return rc;
    if ((rc = ix->lex_stat.grow((size_t)m + 1)) != CSS_OK) return rc;
    std::vector<long long> out((size_t)m + 1);
    if (m) CSS_HIP_TRY(hipMemcpyAsync(ix->lex_ask.p, terms_host, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lex_stats, dim3((unsigned)(m / 256 + 1)), dim3(256), 0, st, (const uint32_t*)ix->lex_ask.p, m,
                       (const uint32_t*)ix->lex_df.p, (const unsigned long long*)ix->lex_total.p, ix->lex_stat.p);
    CSS_LAUNCH_CHECK();
    CSS_HIP_TRY(hipMemcpyAsync(out.data(), ix->lex_stat.p, ((size_t)m + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    for (int j = 0; j < m; ++j) df_out[j] = out[(size_t)j];
    *total_len_out = out[(size_t)m];
    return CSS_OK;
}

namespace {
// word w of a host bitmap cut to the rows [0, T) (null: every row)
inline uint32_t sig_word(const uint32_t* bits, int64_t w, int64_t T) {
    uint32_t v = bits ? bits[w] : 0xFFFFFFFFu;
    if ((w + 1) * 32 > T) v &= (uint32_t)((1ull << (T - w * 32)) - 1ull);
    return v;
}
inline int64_t sig_popcount(const uint32_t* bits, int64_t T) {
    if (!bits) return T;
    int64_t n = 0;
    for (int64_t w = 0, words = (T + 31) / 32; w < words; ++w) n += __builtin_popcount(sig_word(bits, w, T));
    return n;
}
// the first row below T that `a` selects and `b` does not (-1: none)
inline int64_t sig_first_outside(const uint32_t* a, const uint32_t* b, int64_t T) {
    if (!b) return -1;
    for (int64_t w = 0, words = (T + 31) / 32; w < words; ++w) {
        const uint32_t bad = sig_word(a, w, T) & ~b[w];
        if (bad) return w * 32 + __builtin_ctz(bad);
    }
    return -1;
}

// table[t] = the rows r < T with mask bit r (null: every row) whose list holds t.  Enqueued on `st`.
int sig_count_enqueue(css_index* ix, const uint32_t* mask_dev, int64_t T, int64_t ntotal, uint32_t* table, hipStream_t st) {
    {
        ProfScope pz("sig_zero", st);
        CSS_HIP_TRY(hipMemsetAsync(table, 0, (size_t)CSS_TERM_SPACE * sizeof(uint32_t), st));
    }
    const int slots = ix->sig_slots < 0 ? kSigMaxSlots : ix->sig_slots;
    int shift = 32;
    for (int s = slots; s > 1; s >>= 1) --shift;
    // one block of 16 waves per CU that strides over the 1024-row groups: the fewer blocks, the more repeats one LDS
    // table merges and the fewer adds the flushes send to the addresses of the frequent terms
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((T + 64 * kSigWaves - 1) / (64 * kSigWaves), (int64_t)ix->num_cus));
    ProfScope ps("sig_count", st);
    hipLaunchKernelGGL(k_sig_count, dim3((unsigned)blocks), dim3(64 * kSigWaves), (size_t)slots * 2 * sizeof(uint32_t), st,
                       (const uint32_t*)ix->lex_ent.p, (const int64_t*)ix->lex_off.p, T, ntotal, mask_dev, slots, shift, table);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

int sig_state_reset(css_index* ix, hipStream_t st) {
    const size_t words = (sizeof(SigState) + 7) / 8;
    int rc;
    if ((rc = ix->sig_st.grow_exact(words, "hipMalloc(significant terms)")) != CSS_OK) return rc;
    CSS_HIP_TRY(hipMemsetAsync(ix->sig_st.p, 0, words * 8, st));
    return CSS_OK;
}

// css_index_subset_terms under the call's frame; T rows have lists and at least one of them is selected
int subset_terms_locked(css_index* ix, HostCall& hc, const uint32_t* allow_bits_host, int64_t T, int64_t cap,
                        uint32_t* terms_out, int64_t* fg_out, int64_t* n_out) {
    const hipStream_t st = ix->stream;
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if ((rc = ix->sig_fg.grow_exact((size_t)CSS_TERM_SPACE, "hipMalloc(significant terms)")) != CSS_OK) return rc;
    hc.enqueued = true;
    if ((rc = upload_allow_bits(ix, allow_bits_host, &hc.rows)) != CSS_OK) return rc;
    if ((rc = sig_count_enqueue(ix, hc.rows.mask, T, hc.rows.n, ix->sig_fg.p, st)) != CSS_OK) return rc;
    if ((rc = sig_state_reset(ix, st)) != CSS_OK) return rc;
    SigState* ss = reinterpret_cast<SigState*>(ix->sig_st.p);
    hipLaunchKernelGGL(k_sig_nz_count, dim3(kSigBlocks), dim3(256), 0, st, (const uint32_t*)ix->sig_fg.p, ss);
    CSS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sig_nz_scan, dim3(1), dim3(256), 0, st, ss);
    CSS_LAUNCH_CHECK();
    uint32_t total = 0;
    CSS_HIP_TRY(hipMemcpyAsync(&total, &ss->total, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    *n_out = (int64_t)total;
    if (total == 0 || cap < (int64_t)total) return CSS_OK;   // (sizing call, or a buffer too small: nothing is written)
    if ((rc = ix->sig_term.grow((size_t)total)) != CSS_OK) return rc;
    if ((rc = ix->sig_cnt.grow((size_t)total)) != CSS_OK) return rc;
    hipLaunchKernelGGL(k_sig_compact, dim3(kSigBlocks), dim3(256), 0, st, (const uint32_t*)ix->sig_fg.p, (const SigState*)ss, total,
                       ix->sig_term.p, ix->sig_cnt.p);
    CSS_LAUNCH_CHECK();
    std::vector<uint32_t> cnt((size_t)total);
    CSS_HIP_TRY(hipMemcpyAsync(terms_out, ix->sig_term.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipMemcpyAsync(cnt.data(), ix->sig_cnt.p, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < total; ++i) fg_out[i] = (int64_t)cnt[i];
    return CSS_OK;
}

// css_index_significant_terms under the call's frame; FG >= 1 rows are selected, BG >= FG form the background
int significant_terms_locked(css_index* ix, HostCall& hc, const uint32_t* allow_bits_host, const uint32_t* background_bits_host,
                             int64_t T, int64_t FG, int64_t BG, int m, uint32_t min_count, unsigned long long* packed) {
    const hipStream_t st = ix->stream;
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if ((rc = ix->sig_fg.grow_exact((size_t)CSS_TERM_SPACE, "hipMalloc(significant terms)")) != CSS_OK) return rc;
    const uint32_t* bg = ix->lex_df.p;   // no background mask: every row below T, which is what df counts
    if (background_bits_host) {
        const size_t words = (size_t)((hc.rows.n + 31) / 32);
        if ((rc = ix->sig_bg.grow_exact((size_t)CSS_TERM_SPACE, "hipMalloc(significant terms)")) != CSS_OK) return rc;
        if ((rc = ix->sig_mask2.grow(words)) != CSS_OK) return rc;
        bg = ix->sig_bg.p;
    }
    // the candidates: at most one per distinct term of the lists
    const uint32_t cap = (uint32_t)std::min<int64_t>((int64_t)CSS_TERM_SPACE, std::max<int64_t>(ix->lex_off_h[(size_t)T], 1));
    if ((rc = ix->sig_key.grow((size_t)cap)) != CSS_OK) return rc;
    if ((rc = ix->sig_term.grow((size_t)cap)) != CSS_OK) return rc;
    constexpr size_t out_words = CSS_MAX_SIG_TERMS + 3 * CSS_MAX_SIG_TERMS / 2 + 1;
    if ((rc = ix->sig_out.grow_exact(out_words, "hipMalloc(significant terms)")) != CSS_OK) return rc;
    hc.enqueued = true;
    if ((rc = upload_allow_bits(ix, allow_bits_host, &hc.rows)) != CSS_OK) return rc;
    if ((rc = sig_count_enqueue(ix, hc.rows.mask, T, hc.rows.n, ix->sig_fg.p, st)) != CSS_OK) return rc;
    if (background_bits_host) {
        CSS_HIP_TRY(hipMemcpyAsync(ix->sig_mask2.p, background_bits_host, (size_t)((hc.rows.n + 31) / 32) * sizeof(uint32_t),
                                   hipMemcpyHostToDevice, st));
        if ((rc = sig_count_enqueue(ix, ix->sig_mask2.p, T, hc.rows.n, ix->sig_bg.p, st)) != CSS_OK) return rc;
    }
    if ((rc = sig_state_reset(ix, st)) != CSS_OK) return rc;
    SigState* ss = reinterpret_cast<SigState*>(ix->sig_st.p);
    const unsigned grid = (unsigned)std::max(1, ix->num_cus * 8);
    {
        ProfScope ps("sig_select", st);
        hipLaunchKernelGGL(k_sig_score, dim3(grid), dim3(256), 0, st, (const uint32_t*)ix->sig_fg.p, bg, (unsigned long long)FG,
                           (unsigned long long)BG, min_count, cap, ix->sig_key.p, ix->sig_term.p, ss);
        CSS_LAUNCH_CHECK();
        const unsigned sgrid = (unsigned)std::max(1, ix->num_cus * 2);
        for (int d = 0; d < kSigDigits; ++d) {
            hipLaunchKernelGGL(k_sig_hist, dim3(sgrid), dim3(256), 0, st, (const unsigned long long*)ix->sig_key.p,
                               (const uint32_t*)ix->sig_term.p, cap, d, ss);
            CSS_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_sig_pick, dim3(1), dim3(64), 0, st, d, (uint32_t)m, cap, ss);
            CSS_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_sig_gather, dim3(sgrid), dim3(256), 0, st, (const unsigned long long*)ix->sig_key.p,
                           (const uint32_t*)ix->sig_term.p, cap, ss);
        CSS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sig_final, dim3(1), dim3(CSS_MAX_SIG_TERMS), 0, st, (const uint32_t*)ix->sig_fg.p, bg, (const SigState*)ss,
                           ix->sig_out.p);
        CSS_LAUNCH_CHECK();
    }
    CSS_HIP_TRY(hipMemcpyAsync(packed, ix->sig_out.p, out_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    CSS_HIP_TRY(hipStreamSynchronize(st));   // one wait
    return CSS_OK;
}
}  // namespace

int css_index_subset_terms(css_index* ix, const uint32_t* allow_bits_host, int64_t cap, uint32_t* terms_out, int64_t* fg_out,
                           int64_t* n_out, int64_t* rows_out) {
    CSS_REQUIRE(ix, "css_index_subset_terms: NULL index");
    CSS_REQUIRE(n_out && rows_out, "css_index_subset_terms: NULL buffer");
    CSS_REQUIRE(cap >= 0 && (cap == 0 || (terms_out && fg_out)), "css_index_subset_terms: cap=%lld without buffers", (long long)cap);
    HostCall hc(ix, nullptr, false);
    *n_out = 0;
    *rows_out = 0;
    const int64_t T = std::min(ix->lex_rows, hc.rows.n);
    if (T == 0) return CSS_OK;
    const int64_t FG = sig_popcount(allow_bits_host, T);
    *rows_out = FG;
    if (FG == 0) return CSS_OK;
    return hc.wait_if_failed(subset_terms_locked(ix, hc, allow_bits_host, T, cap, terms_out, fg_out, n_out));
}

int css_index_significant_terms(css_index* ix, const uint32_t* allow_bits_host, const uint32_t* background_bits_host, int m,
                                int64_t min_count, uint32_t* terms_out, int64_t* fg_out, int64_t* bg_out, double* score_out,
                                int* n_out, int64_t* fg_rows_out, int64_t* bg_rows_out) {
    CSS_REQUIRE(ix, "css_index_significant_terms: NULL index");
    CSS_REQUIRE(m >= 1 && m <= CSS_MAX_SIG_TERMS, "css_index_significant_terms: m=%d outside [1, %d]", m, CSS_MAX_SIG_TERMS);
    CSS_REQUIRE(min_count >= 1, "css_index_significant_terms: min_count=%lld is below 1", (long long)min_count);
    CSS_REQUIRE(terms_out && fg_out && bg_out && score_out && n_out && fg_rows_out && bg_rows_out,
                "css_index_significant_terms: NULL buffer");
    HostCall hc(ix, nullptr, false);
    const int64_t T = std::min(ix->lex_rows, hc.rows.n);
    const int64_t outside = sig_first_outside(allow_bits_host, background_bits_host, T);
    CSS_REQUIRE(outside < 0, "css_index_significant_terms: row %lld is selected but not in the background", (long long)outside);
    for (int i = 0; i < m; ++i) {
        terms_out[i] = kSigEmpty;
        fg_out[i] = bg_out[i] = 0;
        score_out[i] = 0.0;
    }
    *n_out = 0;
    *fg_rows_out = *bg_rows_out = 0;
    if (T == 0) return CSS_OK;
    const int64_t FG = sig_popcount(allow_bits_host, T), BG = sig_popcount(background_bits_host, T);
    if (FG == 0) return CSS_OK;
    *fg_rows_out = FG;
    *bg_rows_out = BG;
    constexpr int N = CSS_MAX_SIG_TERMS;
    unsigned long long packed[N + 3 * N / 2 + 1];
    const uint32_t mc = (uint32_t)std::min<int64_t>(min_count, 0xFFFFFFFFll);
    const int rc = significant_terms_locked(ix, hc, allow_bits_host, background_bits_host, T, FG, BG, m, mc, packed);
    if (rc != CSS_OK) return hc.wait_if_failed(rc);
    const uint32_t* terms = reinterpret_cast<const uint32_t*>(packed + N);
    const int n = (int)packed[N + 3 * N / 2];
    for (int i = 0; i < n; ++i) {
        terms_out[i] = terms[i];
        fg_out[i] = (int64_t)terms[N + i];
        bg_out[i] = (int64_t)terms[2 * N + i];
        memcpy(&score_out[i], &packed[i], sizeof(double));
    }
    *n_out = n;
    return CSS_OK;
}

namespace {
// What css_index_search_hybrid uploads in ONE copy (floats of q_raw): the query, then the terms and their weights
inline size_t hybrid_terms_at(const css_index* ix) { return ((size_t)ix->dim + 3) / 4 * 4; }

// The column of a hybrid call: BM25 over the term lists (k1, b, avgdl) or the dot product with the sparse vectors
enum class ColumnKind { Bm25, Sparse };
struct LexQuery {
    int m;
    float alpha, k1, b, avgdl;
    ColumnKind kind = ColumnKind::Bm25;
    int max_terms() const { return kind == ColumnKind::Sparse ? CSS_MAX_SPARSE_QUERY_TERMS : CSS_MAX_QUERY_TERMS; }
    int64_t list_rows(const css_index* ix) const { return kind == ColumnKind::Sparse ? ix->sp_rows : ix->lex_rows; }
};

// The dot column of one query (m >= 1 terms and weights on the device) over the sparse vectors of rows.n > 0 rows into
// `col`; rows without a common term, and rows beyond the vectors, get `miss`.  Enqueued on `st`.
int sparse_scores_enqueue(css_index* ix, const Rows& rows, const uint32_t* qterms, const float* qweights, int m, float miss,
                          float* col, hipStream_t st) {
    const int64_t T = std::min(ix->sp_rows, rows.n);
    const unsigned long long* ent = ix->sp_ent.p;
    const int64_t* off = ix->sp_off.p;
    ProfScope ps("sparse_scores", st);
    if (m <= 32)
        hipLaunchKernelGGL((k_sparse_scores<32, 4, 64, 4>), dim3((unsigned)((rows.n + 255) / 256)), dim3(256), 0, st, ent, off, T, rows.n,
                           qterms, qweights, m, miss, col);
    else
        hipLaunchKernelGGL((k_sparse_scores<64, 4, 32, 4>), dim3((unsigned)((rows.n + 127) / 128)), dim3(256), 0, st, ent, off, T, rows.n,
                           qterms, qweights, m, miss, col);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// The call's column (where it has one), search_prior_enqueue on a COPY of the rows whose priors point at it,
// and L behind them.  Everything is enqueued on `st`; nothing waits for the device.  Caller holds ws_mu and a shared
// lock on mu.
int search_hybrid_enqueue(css_index* ix, const Rows& rows, const float* in_dev, const LexQuery& lq, int k, int normalize_q,
                          float* D_dev, int64_t* I_dev, float* S_dev, float* L_dev, hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    Rows fused = rows;
    fused.priors = nullptr;   // (the stored priors play no part in this call)
    const bool lexical = lq.m > 0 && lq.alpha != 0.f && lq.list_rows(ix) > 0 && rows.n > 0;
    if (lexical) {
        if ((rc = ix->lex_col.grow((size_t)rows.n)) != CSS_OK) return rc;
        const uint32_t* qterms = reinterpret_cast<const uint32_t*>(in_dev + hybrid_terms_at(ix));
        const float* qweights = in_dev + hybrid_terms_at(ix) + lq.max_terms();
        if (lq.kind == ColumnKind::Sparse) {
            if ((rc = sparse_scores_enqueue(ix, rows, qterms, qweights, lq.m, 0.0f, ix->lex_col.p, st)) != CSS_OK) return rc;
        } else {
            const float c0 = lq.k1 * (1.0f - lq.b), c1 = (lq.k1 * lq.b) / lq.avgdl;
            ProfScope ps("lex_scores", st);
            hipLaunchKernelGGL(k_lex_scores, dim3((unsigned)((rows.n + 64 * kWaves - 1) / (64 * kWaves))), dim3(256), 0, st,
                               (const uint32_t*)ix->lex_ent.p, (const int64_t*)ix->lex_off.p, (const uint32_t*)ix->lex_dl.p,
                               std::min(ix->lex_rows, rows.n), rows.n, qterms, qweights, lq.m, lq.k1, c0, c1, ix->lex_col.p);
            CSS_LAUNCH_CHECK();
        }
        fused.priors = ix->lex_col.p;
    }
    if ((rc = search_prior_enqueue(ix, fused, in_dev, 1, k, lexical ? lq.alpha : 0.f, normalize_q, D_dev, I_dev, S_dev, st)) != CSS_OK)
        return rc;
    hipLaunchKernelGGL(k_lex_gather, dim3(1), dim3(128), 0, st, (const int64_t*)I_dev, k, rows.id_base, fused.priors, L_dev);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}
}  // namespace

int css_index_search_hybrid(css_index* ix, const float* q_host, int k, float alpha, const uint32_t* terms_host,
                            const float* weights_host, int m, float k1, float b, float avgdl, int normalize_q,
                            const uint32_t* allow_bits_host, float* D_host, int64_t* I_host, float* S_host, float* L_host) {
    CSS_REQUIRE(ix, "css_index_search_hybrid: NULL index");
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "css_index_search_hybrid: k=%d outside [1, %d]", k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(m >= 0 && m <= CSS_MAX_QUERY_TERMS, "css_index_search_hybrid: m=%d outside [0, %d]", m, CSS_MAX_QUERY_TERMS);
    CSS_REQUIRE(std::isfinite(alpha), "css_index_search_hybrid: alpha is %s (it must be finite)", std::isnan(alpha) ? "NaN" : "infinite");
    CSS_REQUIRE(std::isfinite(k1) && k1 >= 0.f, "css_index_search_hybrid: k1 is %s (it must be finite and >= 0)",
                std::isnan(k1) ? "NaN" : std::isinf(k1) ? "infinite" : "negative");
    CSS_REQUIRE(std::isfinite(b) && b >= 0.f && b <= 1.f, "css_index_search_hybrid: b is %s (it must lie in [0, 1])",
                std::isnan(b) ? "NaN" : std::isinf(b) ? "infinite" : "outside [0, 1]");
    CSS_REQUIRE(std::isfinite(avgdl) && avgdl > 0.f, "css_index_search_hybrid: avgdl is %s (it must be finite and > 0)",
                std::isnan(avgdl) ? "NaN" : std::isinf(avgdl) ? "infinite" : "not positive");
    CSS_REQUIRE(q_host && D_host && I_host && (m == 0 || (terms_host && weights_host)), "css_index_search_hybrid: NULL buffer");
    for (int j = 0; j < m; ++j) {
        CSS_REQUIRE(terms_host[j] < CSS_TERM_SPACE, "css_index_search_hybrid: term %u (number %d) is outside [0, 2^24)", terms_host[j], j);
        CSS_REQUIRE(std::isfinite(weights_host[j]), "css_index_search_hybrid: the weight of term %u (number %d) is %s (weights are finite)",
                    terms_host[j], j, std::isnan(weights_host[j]) ? "NaN" : "infinite");
        for (int i = 0; i < j; ++i)
            CSS_REQUIRE(terms_host[i] != terms_host[j], "css_index_search_hybrid: term %u is repeated (numbers %d and %d)",
                        terms_host[j], i, j);
    }
    HostCall hc(ix);
    // the ONE upload: the query, the terms, the weights
    const size_t at = hybrid_terms_at(ix);
    std::vector<float> in(at + 2 * CSS_MAX_QUERY_TERMS, 0.f);
    memcpy(in.data(), q_host, (size_t)ix->dim * sizeof(float));
    if (m) memcpy(in.data() + at, terms_host, (size_t)m * sizeof(uint32_t));
    if (m) memcpy(in.data() + at + CSS_MAX_QUERY_TERMS, weights_host, (size_t)m * sizeof(float));
    hc.cols = 2;   // [S | L]
    int rc = hc.upload(allow_bits_host, ix->q_raw, (const float*)in.data(), in.size(), (size_t)k, &ix->hyb_sl);
    if (rc == CSS_OK) {
        float* sl = reinterpret_cast<float*>(hc.g_out);
        rc = search_hybrid_enqueue(ix, hc.rows, ix->q_raw.p, LexQuery{m, alpha, k1, b, avgdl}, k, normalize_q, hc.d_out, hc.i_out,
                                   sl, sl + k, ix->stream);
    }
    float sl_host[2 * CSS_KERNEL_MAX_K];
    rc = hc.finish(rc, D_host, I_host, reinterpret_cast<int32_t*>(sl_host));
    if (rc != CSS_OK) return rc;
    if (S_host) memcpy(S_host, sl_host, (size_t)k * sizeof(float));
    if (L_host) memcpy(L_host, sl_host + k, (size_t)k * sizeof(float));
    return CSS_OK;
}

// ------------------------------------------------------------------ per-row sparse vectors and sparse search
int css_index_set_sparse(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host, const uint32_t* terms_host,
                         const float* weights_host) {
    CSS_REQUIRE(ix, "css_index_set_sparse: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);   // (ws_pending)
    const int64_t T0 = ix->sp_rows;
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "css_index_set_sparse: rows [%lld, %lld + %lld) outside [0, %lld)",
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(row0 <= T0, "css_index_set_sparse: row0=%lld beyond the %lld rows that have vectors (vectors are append-only)",
                (long long)row0, (long long)T0);
    CSS_REQUIRE(n == 0 || offsets_host, "css_index_set_sparse: offsets is NULL");
    // everything is looked at before anything is written
    if (n > 0) {
        CSS_REQUIRE(offsets_host[0] == 0, "css_index_set_sparse: offsets start at %lld, not 0", (long long)offsets_host[0]);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t c = offsets_host[i + 1] - offsets_host[i];
            CSS_REQUIRE(c >= 0, "css_index_set_sparse: offsets decrease at row %lld", (long long)(row0 + i));
            CSS_REQUIRE(c <= CSS_MAX_SPARSE_ROW_ENTRIES, "css_index_set_sparse: row %lld has %lld entries (at most %d)",
                        (long long)(row0 + i), (long long)c, CSS_MAX_SPARSE_ROW_ENTRIES);
        }
        CSS_REQUIRE(offsets_host[n] == 0 || (terms_host && weights_host), "css_index_set_sparse: terms or weights is NULL");
        for (int64_t i = 0; i < n; ++i)
            for (int64_t t = offsets_host[i]; t < offsets_host[i + 1]; ++t) {
                CSS_REQUIRE(terms_host[t] < CSS_TERM_SPACE, "css_index_set_sparse: term %u of row %lld is outside [0, 2^24)",
                            terms_host[t], (long long)(row0 + i));
                const float w = weights_host[t];
                CSS_REQUIRE(std::isfinite(w) && w > 0.f && w <= CSS_MAX_SPARSE_WEIGHT,
                            "css_index_set_sparse: the weight of term %u of row %lld is %s (weights are finite, > 0 and <= 65536)",
                            terms_host[t], (long long)(row0 + i),
                            std::isnan(w) ? "NaN" : std::isinf(w) ? "infinite" : w > 0.f ? "too large" : w == 0.f ? "zero" : "negative");
            }
    }
    if (n == 0 && row0 == T0) return CSS_OK;
    // each row sorted on the host: term | weight bits << 32, ascending by term (a repeated term shows as neighbours)
    std::vector<unsigned long long> ent;
    std::vector<int64_t> off;
    const int64_t E0 = T0 > 0 ? ix->sp_off_h[(size_t)row0] : 0;
    try {
        ent.reserve(n > 0 ? (size_t)offsets_host[n] : 0);
        off.resize((size_t)n + 1);
        off[0] = E0;
        for (int64_t i = 0; i < n; ++i) {
            const size_t a = ent.size();
            for (int64_t t = offsets_host[i]; t < offsets_host[i + 1]; ++t) {
                uint32_t bits;
                memcpy(&bits, &weights_host[t], sizeof bits);
                ent.push_back((unsigned long long)bits << 32 | terms_host[t]);
            }
            std::sort(ent.begin() + (ptrdiff_t)a, ent.end(),
                      [](unsigned long long x, unsigned long long y) { return (uint32_t)x < (uint32_t)y; });
            for (size_t e = a + 1; e < ent.size(); ++e)
                CSS_REQUIRE((uint32_t)ent[e] != (uint32_t)ent[e - 1], "css_index_set_sparse: term %u is repeated in row %lld",
                            (uint32_t)ent[e], (long long)(row0 + i));
            off[(size_t)i + 1] = E0 + (int64_t)ent.size();
        }
        ix->sp_off_h.reserve((size_t)(row0 + n) + 1);
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_set_sparse: out of host memory");
        return CSS_ERR_OOM;
    }
    DeviceGuard g(ix->device);
    const hipStream_t st = ix->stream;
    // as css_index_set_terms: a search on another stream may still read the vectors that go or move
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if (ix->ws_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ws_ev, 0));
    int rc;
    if (ix->sp_off_h.empty()) ix->sp_off_h.assign(1, 0);   // first vectors of this index
    if (row0 < T0) {   // the vectors of rows >= row0 go
        ix->sp_off_h.resize((size_t)row0 + 1);
        ix->sp_rows = row0;
    }
    if (n > 0) {
        const size_t nE = ent.size();
        if ((rc = grow_keep(ix, ix->sp_ent, (size_t)E0, (size_t)E0 + std::max<size_t>(nE, 1), "hipMalloc(sparse vectors)")) != CSS_OK) return rc;
        if ((rc = grow_keep(ix, ix->sp_off, (size_t)row0 + 1, (size_t)(row0 + n) + 1, "hipMalloc(sparse vectors)")) != CSS_OK) return rc;
        if (nE) CSS_HIP_TRY(hipMemcpyAsync(ix->sp_ent.p + E0, ent.data(), nE * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        CSS_HIP_TRY(hipMemcpyAsync(ix->sp_off.p + row0, off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    CSS_HIP_TRY(hipStreamSynchronize(st));   // (the copies read this call's vectors)
    ix->sp_off_h.insert(ix->sp_off_h.end(), off.begin() + 1, off.end());
    ix->sp_rows = row0 + n;
    return CSS_OK;
}

int css_index_get_sparse(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out, uint32_t* terms_out, float* weights_out) {
    CSS_REQUIRE(ix, "css_index_get_sparse: NULL index");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "css_index_get_sparse: rows [%lld, %lld + %lld) outside [0, %lld)",
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(offsets_out, "css_index_get_sparse: offsets_out is NULL");
    const int64_t T = ix->sp_rows;
    const int64_t a = std::min(row0, T), e = std::min(row0 + n, T);   // the rows of the range that have vectors
    const int64_t E0 = T > 0 ? ix->sp_off_h[(size_t)a] : 0;
    for (int64_t i = 0; i <= n; ++i) offsets_out[i] = T > 0 ? ix->sp_off_h[(size_t)std::min(row0 + i, T)] - E0 : 0;
    const int64_t nE = offsets_out[n];
    if (e <= a || nE == 0 || !(terms_out || weights_out)) return CSS_OK;
    std::vector<unsigned long long> ent;
    try {
        ent.resize((size_t)nE);
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_get_sparse: out of host memory");
        return CSS_ERR_OOM;
    }
    DeviceGuard g(ix->device);
    CSS_HIP_TRY(hipMemcpy(ent.data(), ix->sp_ent.p + E0, (size_t)nE * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nE; ++i) {
        if (terms_out) terms_out[i] = (uint32_t)ent[(size_t)i];
        const uint32_t bits = (uint32_t)(ent[(size_t)i] >> 32);
        if (weights_out) memcpy(&weights_out[i], &bits, sizeof bits);
    }
    return CSS_OK;
}

int css_index_sparse_rows(css_index* ix, int64_t* rows_out) {
    CSS_REQUIRE(ix && rows_out, "css_index_sparse_rows: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    *rows_out = ix->sp_rows;
    return CSS_OK;
}

namespace {
// the checks that css_index_search_sparse and css_index_search_hybrid_sparse make of a sparse query
int sparse_query_check(const char* fn, const uint32_t* terms_host, const float* weights_host, int m) {
    CSS_REQUIRE(m >= 0 && m <= CSS_MAX_SPARSE_QUERY_TERMS, "%s: m=%d outside [0, %d]", fn, m, CSS_MAX_SPARSE_QUERY_TERMS);
    CSS_REQUIRE(m == 0 || (terms_host && weights_host), "%s: NULL buffer", fn);
    for (int j = 0; j < m; ++j) {
        const float w = weights_host[j];
        CSS_REQUIRE(terms_host[j] < CSS_TERM_SPACE, "%s: term %u (number %d) is outside [0, 2^24)", fn, terms_host[j], j);
        CSS_REQUIRE(std::isfinite(w) && w != 0.f && fabsf(w) <= CSS_MAX_SPARSE_WEIGHT,
                    "%s: the weight of term %u (number %d) is %s (weights are finite, nonzero and at most 65536 in size)", fn,
                    terms_host[j], j, std::isnan(w) ? "NaN" : std::isinf(w) ? "infinite" : w == 0.f ? "zero" : "too large");
        for (int i = 0; i < j; ++i)
            CSS_REQUIRE(terms_host[i] != terms_host[j], "%s: term %u is repeated (numbers %d and %d)", fn, terms_host[j], i, j);
    }
    return CSS_OK;
}

// rows per block of k_sparse_topk over n > 0 rows: at least kSparseTopkMinSlice, a multiple of 256, at most
// kSparseTopkMaxParts blocks
inline int64_t sparse_topk_slice(int64_t n) {
    const int64_t per = (n + kSparseTopkMaxParts - 1) / kSparseTopkMaxParts;
    return std::max<int64_t>(kSparseTopkMinSlice, (per + 255) / 256 * 256);
}

// The dot column with miss = -inf, its top-k by slices, and the part merge.  `in_dev`: [64 terms | 64 weights].
// Everything is enqueued on `st`; nothing waits for the device.  Caller holds ws_mu and a shared lock on mu.
int search_sparse_enqueue(css_index* ix, const Rows& rows, const float* in_dev, int m, int k, float* D_dev, int64_t* I_dev,
                          hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if (m == 0 || ix->sp_rows == 0 || rows.n == 0) {
        hipLaunchKernelGGL(k_sparse_pad, dim3(1), dim3(128), 0, st, D_dev, I_dev, k);
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    CSS_REQUIRE(rows.n < 0xFFFFFFFFll, "css_index_search_sparse: %lld rows exceed the 32-bit row numbers of the lists",
                (long long)rows.n);
    // rows appended on another stream must have landed (the mask and the row count speak of them)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    const int64_t slice = sparse_topk_slice(rows.n);
    const int parts = (int)((rows.n + slice - 1) / slice);
    if ((rc = ix->lex_col.grow((size_t)rows.n)) != CSS_OK) return rc;
    if ((rc = ix->sp_pd.grow((size_t)parts * k)) != CSS_OK) return rc;
    if ((rc = ix->sp_pi.grow((size_t)parts * k)) != CSS_OK) return rc;
    if ((rc = sparse_scores_enqueue(ix, rows, reinterpret_cast<const uint32_t*>(in_dev), in_dev + CSS_MAX_SPARSE_QUERY_TERMS, m,
                                    -INFINITY, ix->lex_col.p, st)) != CSS_OK)
        return rc;
    {
        ProfScope ps("sparse_topk", st);
        hipLaunchKernelGGL(k_sparse_topk, dim3((unsigned)parts), dim3(256), 0, st, (const float*)ix->lex_col.p, rows.n, slice,
                           rows.mask, k, rows.id_base, ix->sp_pd.p, ix->sp_pi.p);
        CSS_LAUNCH_CHECK();
    }
    // (larger is better whatever the index's metric: the parts merge as inner-product lists)
    return merge_parts(ix->sp_pd.p, ix->sp_pi.p, parts, k, k, 1, k, CSS_METRIC_IP, D_dev, I_dev, ix->device, st,
                       "css_index_search_sparse");
}
}  // namespace

int css_index_search_sparse(css_index* ix, const uint32_t* terms_host, const float* weights_host, int m, int k,
                            const uint32_t* allow_bits_host, float* D_host, int64_t* I_host) {
    CSS_REQUIRE(ix, "css_index_search_sparse: NULL index");
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "css_index_search_sparse: k=%d outside [1, %d]", k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(D_host && I_host, "css_index_search_sparse: NULL buffer");
    int rc = sparse_query_check("css_index_search_sparse", terms_host, weights_host, m);
    if (rc != CSS_OK) return rc;
    HostCall hc(ix);
    // the ONE upload: the terms, the weights
    float in[2 * CSS_MAX_SPARSE_QUERY_TERMS] = {};
    if (m) memcpy(in, terms_host, (size_t)m * sizeof(uint32_t));
    if (m) memcpy(in + CSS_MAX_SPARSE_QUERY_TERMS, weights_host, (size_t)m * sizeof(float));
    rc = hc.upload(allow_bits_host, ix->sp_q, (const float*)in, (size_t)2 * CSS_MAX_SPARSE_QUERY_TERMS, (size_t)k);
    if (rc == CSS_OK) rc = search_sparse_enqueue(ix, hc.rows, ix->sp_q.p, m, k, hc.d_out, hc.i_out, ix->stream);
    return hc.finish(rc, D_host, I_host);
}

int css_index_search_hybrid_sparse(css_index* ix, const float* q_host, int k, float alpha, const uint32_t* terms_host,
                                   const float* weights_host, int m, int normalize_q, const uint32_t* allow_bits_host,
                                   float* D_host, int64_t* I_host, float* S_host, float* L_host) {
    CSS_REQUIRE(ix, "css_index_search_hybrid_sparse: NULL index");
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "css_index_search_hybrid_sparse: k=%d outside [1, %d]", k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(std::isfinite(alpha), "css_index_search_hybrid_sparse: alpha is %s (it must be finite)",
                std::isnan(alpha) ? "NaN" : "infinite");
    CSS_REQUIRE(q_host && D_host && I_host, "css_index_search_hybrid_sparse: NULL buffer");
    int rc = sparse_query_check("css_index_search_hybrid_sparse", terms_host, weights_host, m);
    if (rc != CSS_OK) return rc;
    HostCall hc(ix);
    // the ONE upload: the query, the terms, the weights
    const size_t at = hybrid_terms_at(ix);
    std::vector<float> in(at + 2 * CSS_MAX_SPARSE_QUERY_TERMS, 0.f);
    memcpy(in.data(), q_host, (size_t)ix->dim * sizeof(float));
    if (m) memcpy(in.data() + at, terms_host, (size_t)m * sizeof(uint32_t));
    if (m) memcpy(in.data() + at + CSS_MAX_SPARSE_QUERY_TERMS, weights_host, (size_t)m * sizeof(float));
    hc.cols = 2;   // [S | L]
    rc = hc.upload(allow_bits_host, ix->q_raw, (const float*)in.data(), in.size(), (size_t)k, &ix->hyb_sl);
    if (rc == CSS_OK) {
        float* sl = reinterpret_cast<float*>(hc.g_out);
        rc = search_hybrid_enqueue(ix, hc.rows, ix->q_raw.p, LexQuery{m, alpha, 0.f, 0.f, 1.f, ColumnKind::Sparse}, k, normalize_q,
                                   hc.d_out, hc.i_out, sl, sl + k, ix->stream);
    }
    float sl_host[2 * CSS_KERNEL_MAX_K];
    rc = hc.finish(rc, D_host, I_host, reinterpret_cast<int32_t*>(sl_host));
    if (rc != CSS_OK) return rc;
    if (S_host) memcpy(S_host, sl_host, (size_t)k * sizeof(float));
    if (L_host) memcpy(L_host, sl_host + k, (size_t)k * sizeof(float));
    return CSS_OK;
}

// ------------------------------------------------------------------ per-row token matrices and MaxSim search
namespace {
inline bool bf16_finite(uint16_t v) { return (v & 0x7F80u) != 0x7F80u; }
inline bool token_dim_ok(int P) { return P >= 32 && P <= CSS_MAX_TOKEN_DIM && P % 32 == 0; }
}  // namespace

namespace {
constexpr int64_t kTokCodecPass = 1 << 18;   // tokens of one staging pass of encode / decode (64 MiB of bf16 at P = 128)

// nE raw tokens on the host -> codes and packed buckets from token E0 on, through a staging buffer that dies with the
// call: the raw tokens never stay in HBM.  Enqueued on `st`; the caller waits before `raw` goes.
int tok_encode_enqueue(css_index* ix, const uint16_t* tok_host, int64_t E0, int64_t nE, DevBuf<unsigned short>& raw, hipStream_t st) {
    const size_t P = (size_t)ix->tk_dim, RB = P * (size_t)ix->tk_bits / 8;
    int rc;
    if ((rc = raw.grow_exact((size_t)std::min(nE, kTokCodecPass) * P, "hipMalloc(token staging)")) != CSS_OK) return rc;
    const void* fn = tok_dim((int)P, [](auto p) { return (const void*)k_tok_encode<decltype(p)::value>; });
    for (int64_t c0 = 0; c0 < nE; c0 += kTokCodecPass) {
        int64_t m = std::min(kTokCodecPass, nE - c0);
        CSS_HIP_TRY(hipMemcpyAsync(raw.p, tok_host + (size_t)c0 * P, (size_t)m * P * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        const unsigned short *tok = raw.p, *cent = ix->tk_cent.p;
        const float* cut = ix->tk_cw.p;
        unsigned short* codes = ix->tk_code.p + E0 + c0;
        unsigned char* res = ix->tk_res.p + (size_t)(E0 + c0) * RB;
        int C = ix->tk_ncent, nbits = ix->tk_bits;
        void* args[] = {&tok, &m, &cent, &C, &nbits, &cut, &codes, &res};
        ProfScope ps("tok_encode", st);
        CSS_HIP_TRY(hipLaunchKernel(fn, dim3((unsigned)((m + 64 * kWaves - 1) / (64 * kWaves))), dim3(64 * kWaves), args, 0, st));
    }
    return CSS_OK;
}

// css_index_set_tokens and css_index_set_token_codes: the same rows, rules and bookkeeping.  as_codes: the payload is
// canonical (codes_host, res_host) of the index's codec, stored as it is; otherwise bf16 matrices (tok_host), stored
// raw on an index without a codec and encoded on the device on one that has a codec.
int set_tokens_impl(const char* fn, css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host, const uint16_t* tok_host,
                    int P, bool as_codes, const uint16_t* codes_host, const uint8_t* res_host) {
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);   // (ws_pending)
    const int64_t T0 = ix->tk_rows;
    const int bits = ix->tk_bits;
    if (as_codes) {
        CSS_REQUIRE(bits != 0, "%s: the index has no token codec (css_index_set_token_codec)", fn);
        P = ix->tk_cdim;
    }
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "%s: rows [%lld, %lld + %lld) outside [0, %lld)", fn,
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(row0 <= T0, "%s: row0=%lld beyond the %lld rows that have matrices (matrices are append-only)", fn,
                (long long)row0, (long long)T0);
    CSS_REQUIRE(token_dim_ok(P), "%s: P=%d must be a multiple of 32 in [32, %d]", fn, P, CSS_MAX_TOKEN_DIM);
    CSS_REQUIRE(bits == 0 || n == 0 || P == ix->tk_cdim, "%s: P=%d, but the index's token codec has P=%d", fn, P, ix->tk_cdim);
    CSS_REQUIRE(T0 == 0 || n == 0 || P == ix->tk_dim || row0 == 0,
                "%s: P=%d, but the stored matrices have P=%d (only a rewrite from row 0 changes it)", fn, P, ix->tk_dim);
    CSS_REQUIRE(n == 0 || offsets_host, "%s: offsets is NULL", fn);
    // everything is looked at before anything is written
    if (n > 0) {
        CSS_REQUIRE(offsets_host[0] == 0, "%s: offsets start at %lld, not 0", fn, (long long)offsets_host[0]);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t c = offsets_host[i + 1] - offsets_host[i];
            CSS_REQUIRE(c >= 0, "%s: offsets decrease at row %lld", fn, (long long)(row0 + i));
            CSS_REQUIRE(c <= CSS_MAX_ROW_TOKEN_VECTORS, "%s: row %lld has %lld tokens (at most %d)", fn, (long long)(row0 + i),
                        (long long)c, CSS_MAX_ROW_TOKEN_VECTORS);
        }
        if (as_codes) {
            CSS_REQUIRE(offsets_host[n] == 0 || (codes_host && res_host), "%s: codes or res is NULL", fn);
            for (int64_t i = 0; i < n; ++i)
                for (int64_t e = offsets_host[i]; e < offsets_host[i + 1]; ++e)
                    CSS_REQUIRE((int)codes_host[e] < ix->tk_ncent, "%s: token %lld of row %lld has code %d, the codec has %d centroids",
                                fn, (long long)(e - offsets_host[i]), (long long)(row0 + i), (int)codes_host[e], ix->tk_ncent);
        } else {
            CSS_REQUIRE(offsets_host[n] == 0 || tok_host, "%s: tokens is NULL", fn);
            for (int64_t i = 0; i < n; ++i)
                for (int64_t e = offsets_host[i] * P; e < offsets_host[i + 1] * P; ++e)
                    CSS_REQUIRE(bf16_finite(tok_host[e]), "%s: component %lld of token %lld of row %lld is %s", fn,
                                (long long)(e % P), (long long)(e / P - offsets_host[i]), (long long)(row0 + i),
                                (tok_host[e] & 0x7Fu) ? "NaN" : "infinite");
        }
    }
    if (n == 0 && row0 == T0) return CSS_OK;
    const int64_t E0 = T0 > 0 ? ix->tk_off_h[(size_t)row0] : 0;
    const int64_t nE = n > 0 ? offsets_host[n] : 0;
    std::vector<int64_t> off;
    try {
        off.resize((size_t)n + 1);
        for (int64_t i = 0; i <= n; ++i) off[(size_t)i] = E0 + (n > 0 ? offsets_host[i] : 0);
        ix->tk_off_h.reserve((size_t)(row0 + n) + 1);
    } catch (const std::bad_alloc&) {
        css::set_error("%s: out of host memory", fn);
        return CSS_ERR_OOM;
    }
    DeviceGuard g(ix->device);
    const hipStream_t st = ix->stream;
    // as css_index_set_sparse: a search on another stream may still read the matrices that go or move
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if (ix->ws_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ws_ev, 0));
    int rc;
    if (ix->tk_off_h.empty()) ix->tk_off_h.assign(1, 0);   // first matrices of this index
    if (row0 < T0) {   // the matrices of rows >= row0 go
        ix->tk_off_h.resize((size_t)row0 + 1);
        ix->tk_rows = row0;
    }
    DevBuf<unsigned short> raw;   // (encode's staging: read until the wait below)
    if (n > 0) {
        ix->tk_dim = P;   // (another P only from row 0: nothing of the old width is left)
        const size_t sP = (size_t)P, sE0 = (size_t)E0, sE1 = sE0 + std::max<size_t>((size_t)nE, 1);
        if (bits == 0) {
            if ((rc = grow_keep(ix, ix->tk_tok, sE0 * sP, sE1 * sP, "hipMalloc(token matrices)")) != CSS_OK) return rc;
        } else {
            const size_t RB = sP * (size_t)bits / 8;
            if ((rc = grow_keep(ix, ix->tk_code, sE0, sE1, "hipMalloc(token codes)")) != CSS_OK) return rc;
            if ((rc = grow_keep(ix, ix->tk_res, sE0 * RB, sE1 * RB, "hipMalloc(token codes)")) != CSS_OK) return rc;
        }
        if ((rc = grow_keep(ix, ix->tk_off, (size_t)row0 + 1, (size_t)(row0 + n) + 1, "hipMalloc(token matrices)")) != CSS_OK) return rc;
        if (nE && bits == 0) {
            CSS_HIP_TRY(hipMemcpyAsync(ix->tk_tok.p + sE0 * sP, tok_host, (size_t)nE * sP * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        } else if (nE && as_codes) {
            const size_t RB = sP * (size_t)bits / 8;
            CSS_HIP_TRY(hipMemcpyAsync(ix->tk_code.p + sE0, codes_host, (size_t)nE * sizeof(uint16_t), hipMemcpyHostToDevice, st));
            CSS_HIP_TRY(hipMemcpyAsync(ix->tk_res.p + sE0 * RB, res_host, (size_t)nE * RB, hipMemcpyHostToDevice, st));
        } else if (nE) {
            rc = tok_encode_enqueue(ix, tok_host, E0, nE, raw, st);
            if (rc != CSS_OK) {
                (void)hipStreamSynchronize(st);
                return rc;
            }
        }
        CSS_HIP_TRY(hipMemcpyAsync(ix->tk_off.p + row0, off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    }
    CSS_HIP_TRY(hipStreamSynchronize(st));   // (the copies read this call's matrices)
    ix->tk_off_h.insert(ix->tk_off_h.end(), off.begin() + 1, off.end());
    ix->tk_rows = row0 + n;
    return CSS_OK;
}

// the rows of [row0, row0 + n) that have matrices as offsets from 0; *E0 = their first token, the return their count
int64_t token_range(const css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out, int64_t* E0) {
    const int64_t T = ix->tk_rows;
    const int64_t a = std::min(row0, T);
    *E0 = T > 0 ? ix->tk_off_h[(size_t)a] : 0;
    for (int64_t i = 0; i <= n; ++i) offsets_out[i] = T > 0 ? ix->tk_off_h[(size_t)std::min(row0 + i, T)] - *E0 : 0;
    return offsets_out[n];
}
}  // namespace

int css_index_set_tokens(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host, const uint16_t* tok_host, int P) {
    return set_tokens_impl("css_index_set_tokens", ix, row0, n, offsets_host, tok_host, P, false, nullptr, nullptr);
}

int css_index_set_token_codes(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host, const uint16_t* codes_host,
                              const uint8_t* res_host) {
    return set_tokens_impl("css_index_set_token_codes", ix, row0, n, offsets_host, nullptr, 0, true, codes_host, res_host);
}

int css_index_get_tokens(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out, uint16_t* tok_out) {
    CSS_REQUIRE(ix, "css_index_get_tokens: NULL index");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "css_index_get_tokens: rows [%lld, %lld + %lld) outside [0, %lld)",
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(offsets_out, "css_index_get_tokens: offsets_out is NULL");
    int64_t E0;
    const int64_t nE = token_range(ix, row0, n, offsets_out, &E0);
    if (nE == 0 || !tok_out) return CSS_OK;
    DeviceGuard g(ix->device);
    const size_t P = (size_t)ix->tk_dim;
    if (ix->tk_bits == 0) {
        CSS_HIP_TRY(hipMemcpy(tok_out, ix->tk_tok.p + (size_t)E0 * P, (size_t)nE * P * sizeof(uint16_t), hipMemcpyDeviceToHost));
        return CSS_OK;
    }
    // a compressed store: the DECODED matrices, through a staging buffer of this call
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    const hipStream_t st = ix->stream;
    const size_t RB = P * (size_t)ix->tk_bits / 8;
    DevBuf<unsigned short> raw;
    int rc;
    if ((rc = raw.grow_exact((size_t)std::min(nE, kTokCodecPass) * P, "hipMalloc(token staging)")) != CSS_OK) return rc;
    for (int64_t c0 = 0; c0 < nE; c0 += kTokCodecPass) {
        const int64_t m = std::min(kTokCodecPass, nE - c0);
        const int64_t threads = m * (int64_t)(P / 8);
        hipLaunchKernelGGL(k_tok_decode, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st,
                           (const unsigned short*)ix->tk_code.p + E0 + c0, (const unsigned char*)ix->tk_res.p + (size_t)(E0 + c0) * RB, m,
                           (const unsigned short*)ix->tk_cent.p, (int)P, ix->tk_bits, (const float*)ix->tk_cw.p + 16, raw.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(tok_out + (size_t)c0 * P, raw.p, (size_t)m * P * sizeof(uint16_t), hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);   // (also after a failure: the copy writes this call's memory)
        CSS_HIP_TRY(e);
        CSS_HIP_TRY(e2);
    }
    return CSS_OK;
}

int css_index_get_token_codes(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out, uint16_t* codes_out, uint8_t* res_out) {
    CSS_REQUIRE(ix, "css_index_get_token_codes: NULL index");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    CSS_REQUIRE(ix->tk_bits != 0, "css_index_get_token_codes: the index has no token codec (css_index_set_token_codec)");
    CSS_REQUIRE(row0 >= 0 && n >= 0 && n <= ix->ntotal - row0, "css_index_get_token_codes: rows [%lld, %lld + %lld) outside [0, %lld)",
                (long long)row0, (long long)row0, (long long)n, (long long)ix->ntotal);
    CSS_REQUIRE(offsets_out, "css_index_get_token_codes: offsets_out is NULL");
    int64_t E0;
    const int64_t nE = token_range(ix, row0, n, offsets_out, &E0);
    if (nE == 0 || (!codes_out && !res_out)) return CSS_OK;
    DeviceGuard g(ix->device);
    const size_t RB = (size_t)ix->tk_dim * (size_t)ix->tk_bits / 8;
    if (codes_out) CSS_HIP_TRY(hipMemcpy(codes_out, ix->tk_code.p + E0, (size_t)nE * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (res_out) CSS_HIP_TRY(hipMemcpy(res_out, ix->tk_res.p + (size_t)E0 * RB, (size_t)nE * RB, hipMemcpyDeviceToHost));
    return CSS_OK;
}

int css_index_set_token_codec(css_index* ix, const float* centroids_host, int C, int P, int nbits, const float* cutoffs_host,
                              const float* weights_host) {
    CSS_REQUIRE(ix, "css_index_set_token_codec: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    CSS_REQUIRE(ix->tk_rows == 0, "css_index_set_token_codec: %lld rows have token matrices (the codec changes only while there are none)",
                (long long)ix->tk_rows);
    std::vector<uint16_t> cent_h;
    std::vector<float> cw_h;
    if (centroids_host) {   // everything is checked before anything is allocated
        CSS_REQUIRE(C >= 1 && C <= CSS_MAX_TOKEN_CENTROIDS, "css_index_set_token_codec: C=%d outside [1, %d]", C, CSS_MAX_TOKEN_CENTROIDS);
        CSS_REQUIRE(token_dim_ok(P), "css_index_set_token_codec: P=%d must be a multiple of 32 in [32, %d]", P, CSS_MAX_TOKEN_DIM);
        CSS_REQUIRE(nbits == 1 || nbits == 2 || nbits == 4, "css_index_set_token_codec: nbits=%d is none of 1, 2, 4", nbits);
        CSS_REQUIRE(cutoffs_host && weights_host, "css_index_set_token_codec: cutoffs or weights is NULL");
        const int nw = 1 << nbits;
        for (int i = 0; i < nw - 1; ++i) {
            CSS_REQUIRE(std::isfinite(cutoffs_host[i]), "css_index_set_token_codec: cutoff %d is not finite", i);
            CSS_REQUIRE(i == 0 || cutoffs_host[i - 1] < cutoffs_host[i], "css_index_set_token_codec: cutoff %d does not ascend", i);
        }
        for (int i = 0; i < nw; ++i) CSS_REQUIRE(std::isfinite(weights_host[i]), "css_index_set_token_codec: weight %d is not finite", i);
        try {
            cent_h.resize((size_t)C * P);
            cw_h.assign(32, 0.f);
        } catch (const std::bad_alloc&) {
            css::set_error("css_index_set_token_codec: out of host memory");
            return CSS_ERR_OOM;
        }
        for (size_t e = 0; e < (size_t)C * P; ++e) {
            uint32_t u;
            memcpy(&u, centroids_host + e, sizeof u);
            CSS_REQUIRE((u & 0xFFFFu) == 0, "css_index_set_token_codec: component %d of centroid %d is not a bf16 value (round it first)",
                        (int)(e % P), (int)(e / P));
            CSS_REQUIRE(bf16_finite((uint16_t)(u >> 16)), "css_index_set_token_codec: component %d of centroid %d is %s", (int)(e % P),
                        (int)(e / P), (u & 0x7F0000u) ? "NaN" : "infinite");
            cent_h[e] = (uint16_t)(u >> 16);
        }
        std::copy(cutoffs_host, cutoffs_host + nw - 1, cw_h.begin());
        std::copy(weights_host, weights_host + nw, cw_h.begin() + 16);
    }
    DeviceGuard g(ix->device);
    if (ix->ws_pending) CSS_HIP_TRY(hipEventSynchronize(ix->ws_ev));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    DevBuf<unsigned short> cent;
    DevBuf<float> cw;
    int rc;
    if (centroids_host) {
        if ((rc = cent.grow_exact(cent_h.size(), "hipMalloc(token codec)")) != CSS_OK) return rc;
        if ((rc = cw.grow_exact(cw_h.size(), "hipMalloc(token codec)")) != CSS_OK) return rc;
        CSS_HIP_TRY(hipMemcpy(cent.p, cent_h.data(), cent_h.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        CSS_HIP_TRY(hipMemcpy(cw.p, cw_h.data(), cw_h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if ((rc = drop_tokens(ix)) != CSS_OK) return rc;   // (no rows; buffers of the other storage form may be left)
    ix->tk_cent.swap(cent);
    ix->tk_cw.swap(cw);
    ix->tk_cent_h.swap(cent_h);
    ix->tk_cw_h.swap(cw_h);
    ix->tk_bits = centroids_host ? nbits : 0;
    ix->tk_ncent = centroids_host ? C : 0;
    ix->tk_cdim = centroids_host ? P : 0;
    return CSS_OK;
}

int css_index_get_token_codec(css_index* ix, int* C_out, int* P_out, int* nbits_out, float* centroids_out, float* cutoffs_out,
                              float* weights_out) {
    CSS_REQUIRE(ix, "css_index_get_token_codec: NULL index");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (C_out) *C_out = ix->tk_ncent;
    if (P_out) *P_out = ix->tk_cdim;
    if (nbits_out) *nbits_out = ix->tk_bits;
    if (ix->tk_bits == 0) return CSS_OK;
    const int nw = 1 << ix->tk_bits;
    if (centroids_out)
        for (size_t e = 0; e < ix->tk_cent_h.size(); ++e) {
            const uint32_t u = (uint32_t)ix->tk_cent_h[e] << 16;
            memcpy(centroids_out + e, &u, sizeof u);
        }
    if (cutoffs_out) std::copy(ix->tk_cw_h.begin(), ix->tk_cw_h.begin() + nw - 1, cutoffs_out);
    if (weights_out) std::copy(ix->tk_cw_h.begin() + 16, ix->tk_cw_h.begin() + 16 + nw, weights_out);
    return CSS_OK;
}

int css_index_token_codec_bits(css_index* ix, int* bits_out) {
    CSS_REQUIRE(ix && bits_out, "css_index_token_codec_bits: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    *bits_out = ix->tk_bits;
    return CSS_OK;
}


int css_index_token_rows(css_index* ix, int64_t* rows_out) {
    CSS_REQUIRE(ix && rows_out, "css_index_token_rows: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    *rows_out = ix->tk_rows;
    return CSS_OK;
}

int css_index_token_dim(css_index* ix, int* dim_out) {
    CSS_REQUIRE(ix && dim_out, "css_index_token_dim: NULL argument");
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    *dim_out = ix->tk_rows == 0 ? 0 : ix->tk_dim;
    return CSS_OK;
}

int css_index_drop_tokens(css_index* ix) {
    CSS_REQUIRE(ix, "css_index_drop_tokens: NULL index");
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    if (ix->tk_off_h.empty()) return CSS_OK;
    DeviceGuard g(ix->device);
    // a search on another stream may still read the matrices
    if (ix->ws_pending) CSS_HIP_TRY(hipEventSynchronize(ix->ws_ev));
    CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
    return drop_tokens(ix);
}

int css_index_set_token_blocks(css_index* ix, int blocks) {
    CSS_REQUIRE(ix, "css_index_set_token_blocks: NULL index");
    CSS_REQUIRE(blocks >= 0 && blocks <= 65536, "css_index_set_token_blocks: blocks=%d outside [0, 65536]", blocks);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->tk_blocks = blocks;
    return CSS_OK;
}

namespace {
// The checks that every MaxSim call makes of a query matrix.  The length and the components are two halves, so that
// css_index_search_maxsim_batch makes each of ALL its queries before the next (b >= 0: query b of a batch).
int token_len_check(const char* fn, int64_t mq, int b) {
    if (b < 0) CSS_REQUIRE(mq >= 1 && mq <= CSS_MAX_QUERY_TOKENS, "%s: mq=%d outside [1, %d]", fn, (int)mq, CSS_MAX_QUERY_TOKENS);
    else CSS_REQUIRE(mq >= 1 && mq <= CSS_MAX_QUERY_TOKENS, "%s: query %d has %lld tokens, outside [1, %d]", fn, b, (long long)mq,
                     CSS_MAX_QUERY_TOKENS);
    return CSS_OK;
}
int token_finite_check(const char* fn, const uint16_t* q, int mq, int P, int b) {
    for (int i = 0; i < mq * P; ++i) {
        if (bf16_finite(q[i])) continue;
        const char* what = (q[i] & 0x7Fu) ? "NaN" : "infinite";
        if (b < 0) CSS_REQUIRE(false, "%s: component %d of query token %d is %s", fn, i % P, i / P, what);
        else CSS_REQUIRE(false, "%s: component %d of token %d of query %d is %s", fn, i % P, i / P, b, what);
    }
    return CSS_OK;
}
int token_query_check(const char* fn, const uint16_t* q_tok_host, int mq, int P) {
    const int rc = token_len_check(fn, mq, -1);
    if (rc != CSS_OK) return rc;
    CSS_REQUIRE(token_dim_ok(P), "%s: P=%d must be a multiple of 32 in [32, %d]", fn, P, CSS_MAX_TOKEN_DIM);
    CSS_REQUIRE(q_tok_host, "%s: NULL buffer", fn);
    return token_finite_check(fn, q_tok_host, mq, P, -1);
}

constexpr int kTokGroup = CSS_MAXSIM_BATCH_GROUP;
static_assert(kTokGroup >= 4 && kTokGroup <= 16, "the waves of k_tok_scores_b's block");

// the store as the kernels take it (css_tokens.h): a raw store has tokens, a compressed one codes, packed buckets, the
// centroid table and the 16 weights
TokStore tok_store(const css_index* ix) {
    return TokStore{ix->tk_tok.p, ix->tk_code.p,  ix->tk_res.p, ix->tk_cent.p, ix->tk_bits ? ix->tk_cw.p + 16 : nullptr,
                    ix->tk_off.p, ix->tk_rows};
}

// The grid of a token kernel `fn` (blocks of `threads` threads, `turns` turns at a time per block) over n > 0 rows: as
// many blocks as stay resident (no block waits for another, so the figure only sets the speed), and into *per the rows
// of a turn: kTokTurn for a scan, fewer where that would leave waves idle (per == null: the kernel's turn is always
// kTokTurn rows).  css_index_set_token_blocks fixes the grid and with it kTokTurn rows per turn.
int tok_grid(const css_index* ix, const void* fn, int threads, int64_t n, int turns, int* per, unsigned* grid) {
    int64_t blocks = ix->tk_blocks, rows = kTokTurn;
    if (blocks == 0) {
        int per_cu = 0;
        CSS_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, 0));
        blocks = (int64_t)std::max(per_cu, 1) * ix->num_cus;
        if (per) rows = std::min<int64_t>(kTokTurn, (n + blocks * turns - 1) / (blocks * turns));
    }
    if (per) *per = (int)rows;
    *grid = (unsigned)std::min<int64_t>(blocks, (n + rows * turns - 1) / (rows * turns));
    return CSS_OK;
}

// The MaxSim column of the query (mq tokens of the index's P on the device) over positions [0, n) into `col`: the rows
// 0 .. n - 1 (rows == null; `mask` as in the searches) or the n rows of the list; -inf where the row is a miss.
// n > 0 and the index has matrices.  Enqueued on `st`.
int tok_scores_enqueue(css_index* ix, const uint32_t* rows, int64_t n, const uint32_t* mask, const unsigned short* q, int mq,
                       float* col, hipStream_t st) {
    const void* fn = tok_variant(ix->tk_dim, (mq + 15) / 16, ix->tk_bits, [](auto p, auto mt, auto nb) {
        return (const void*)k_tok_scores<decltype(p)::value, decltype(mt)::value, decltype(nb)::value>;
    });
    int rc, per;
    unsigned grid;
    if ((rc = tok_grid(ix, fn, 64 * kWaves, n, kWaves, &per, &grid)) != CSS_OK) return rc;
    TokStore store = tok_store(ix);
    void* args[] = {&store, &rows, &n, &mask, &q, &mq, &per, &col};
    ProfScope ps(ix->tk_bits ? "tok_scores_c" : "tok_scores", st);
    CSS_HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(64 * kWaves), args, 0, st));
    return CSS_OK;
}

// The MaxSim columns of a group of 2 .. kTokGroup queries (tokens q, offsets qoff [ng + 1] on the device; mq_max: the
// longest of them) over the rows 0 .. n - 1 into col [ng][n].  n > 0 and the index has matrices.  Enqueued on `st`.
int tok_scores_group_enqueue(css_index* ix, int64_t n, const uint32_t* mask, const unsigned short* q, const int64_t* qoff, int ng,
                             int mq_max, float* col, hipStream_t st) {
    const void* fn = tok_variant(ix->tk_dim, (mq_max + 15) / 16, ix->tk_bits, [](auto p, auto mt, auto nb) {
        return (const void*)k_tok_scores_b<decltype(p)::value, decltype(mt)::value, decltype(nb)::value, kTokGroup>;
    });
    int rc;
    unsigned grid;
    if ((rc = tok_grid(ix, fn, 64 * kTokGroup, n, 1, nullptr, &grid)) != CSS_OK) return rc;
    TokStore store = tok_store(ix);
    void* args[] = {&store, &n, &mask, &q, &qoff, &ng, &col};
    ProfScope ps(ix->tk_bits ? "tok_scores_bc" : "tok_scores_b", st);
    CSS_HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(64 * kTokGroup), args, 0, st));
    return CSS_OK;
}

// The frame of the MaxSim searches: nq queries, in groups of at most `group`, over n positions (`mask` and `id_base` as
// in the searches).  Per group, `scores(q0, ng, col)` enqueues the columns [ng][n] of the queries q0 .. q0 + ng - 1
// into `colbuf`; then their top-k by slices and ONE part merge into D_dev / I_dev [q0 ..][k].  An index without
// matrices, or n = 0: the padded answer.  Everything is enqueued on `st`; nothing waits for the device.  Caller holds
// ws_mu, a shared lock on mu and a turn at the workspaces.  (The pruned search comes here behind its candidate step,
// which has made the stream wait for the ingest already: the second wait for the same event is a no-op.)
extern "C++" template <typename F>
int tok_topk_enqueue(css_index* ix, DevBuf<float>& colbuf, int64_t n, const uint32_t* mask, int64_t id_base, int nq, int group,
                     int k, float* D_dev, int64_t* I_dev, const char* who, hipStream_t st, F&& scores) {
    int rc;
    if (ix->tk_rows == 0 || n == 0) {
        const int total = nq * k;
        hipLaunchKernelGGL(k_sparse_pad, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, st, D_dev, I_dev, total);
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    CSS_REQUIRE(n < 0xFFFFFFFFll, "%s: %lld rows exceed the 32-bit row numbers of the lists", who, (long long)n);
    // rows appended on another stream must have landed (the mask and the row count speak of them)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    const int64_t slice = sparse_topk_slice(n);
    const int parts = (int)((n + slice - 1) / slice), gmax = std::min(nq, group);
    if ((rc = colbuf.grow((size_t)n * gmax)) != CSS_OK) return rc;
    if ((rc = ix->sp_pd.grow((size_t)parts * gmax * k)) != CSS_OK) return rc;
    if ((rc = ix->sp_pi.grow((size_t)parts * gmax * k)) != CSS_OK) return rc;
    for (int q0 = 0; q0 < nq; q0 += group) {
        const int ng = std::min(group, nq - q0);
        if ((rc = scores(q0, ng, colbuf.p)) != CSS_OK) return rc;
        {
            ProfScope ps("sparse_topk", st);
            hipLaunchKernelGGL(k_sparse_topk_cols, dim3((unsigned)parts, (unsigned)ng), dim3(256), 0, st, (const float*)colbuf.p, n,
                               slice, mask, k, id_base, ix->sp_pd.p, ix->sp_pi.p);
            CSS_LAUNCH_CHECK();
        }
        // (larger is better whatever the index's metric: the parts merge as inner-product lists)
        if ((rc = merge_parts(ix->sp_pd.p, ix->sp_pi.p, parts, (int64_t)ng * k, (int64_t)ng * k, ng, k, CSS_METRIC_IP,
                              D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, ix->device, st, who)) != CSS_OK) return rc;
    }
    return CSS_OK;
}
}  // namespace

int css_index_search_maxsim(css_index* ix, const uint16_t* q_tok_host, int mq, int P, int k, const uint32_t* allow_bits_host,
                            float* D_host, int64_t* I_host) {
    const char* fn = "css_index_search_maxsim";
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "%s: k=%d outside [1, %d]", fn, k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(D_host && I_host, "%s: NULL buffer", fn);
    int rc = token_query_check(fn, q_tok_host, mq, P);
    if (rc != CSS_OK) return rc;
    HostCall hc(ix);
    CSS_REQUIRE(ix->tk_rows == 0 || P == ix->tk_dim, "%s: the query has P=%d, the stored matrices P=%d", fn, P, ix->tk_dim);
    // the ONE upload: the query matrix
    rc = hc.upload(allow_bits_host, ix->tk_q, (const unsigned short*)q_tok_host, (size_t)mq * P, (size_t)k);
    if (rc == CSS_OK) {
        const hipStream_t st = ix->stream;
        const Rows& rows = hc.rows;
        WsTurn turn(ix, st);
        if ((rc = turn.rc) == CSS_OK)
            rc = tok_topk_enqueue(ix, ix->lex_col, rows.n, rows.mask, rows.id_base, 1, 1, k, hc.d_out, hc.i_out, fn, st,
                                  [&](int, int, float* col) {
                                      return tok_scores_enqueue(ix, nullptr, rows.n, rows.mask, ix->tk_q.p, mq, col, st);
                                  });
    }
    return hc.finish(rc, D_host, I_host);
}

int css_index_search_maxsim_batch(css_index* ix, const uint16_t* q_tok_host, const int64_t* q_offsets_host, int nq, int P, int k,
                                  const uint32_t* allow_bits_host, float* D_host, int64_t* I_host) {
    const char* fn = "css_index_search_maxsim_batch";
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    CSS_REQUIRE(nq >= 1 && nq <= CSS_MAX_MAXSIM_QUERIES, "%s: nq=%d outside [1, %d]", fn, nq, CSS_MAX_MAXSIM_QUERIES);
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "%s: k=%d outside [1, %d]", fn, k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(q_tok_host && q_offsets_host && D_host && I_host, "%s: NULL buffer", fn);
    CSS_REQUIRE(token_dim_ok(P), "%s: P=%d must be a multiple of 32 in [32, %d]", fn, P, CSS_MAX_TOKEN_DIM);
    CSS_REQUIRE(q_offsets_host[0] == 0, "%s: the offsets start at %lld, not at 0", fn, (long long)q_offsets_host[0]);
    int rc;
    for (int b = 0; b < nq; ++b)
        if ((rc = token_len_check(fn, q_offsets_host[b + 1] - q_offsets_host[b], b)) != CSS_OK) return rc;
    for (int b = 0; b < nq; ++b)
        if ((rc = token_finite_check(fn, q_tok_host + (size_t)q_offsets_host[b] * P, (int)(q_offsets_host[b + 1] - q_offsets_host[b]),
                                     P, b)) != CSS_OK) return rc;
    // the ONE upload: [offsets (int64) | the matrices], the matrices behind the offsets at a multiple of 16 bytes
    const size_t ntok = (size_t)q_offsets_host[nq];
    const size_t at = ((size_t)(nq + 1) * 2 + 3) / 4 * 4, q_words = ntok * P / 2;   // (P is even)
    std::vector<uint32_t> in;
    try {
        in.assign(at + q_words, 0u);
    } catch (const std::bad_alloc&) {
        css::set_error("%s: out of host memory", fn);
        return CSS_ERR_OOM;
    }
    memcpy(in.data(), q_offsets_host, (size_t)(nq + 1) * sizeof(int64_t));
    memcpy(in.data() + at, q_tok_host, ntok * P * sizeof(uint16_t));
    HostCall hc(ix);
    CSS_REQUIRE(ix->tk_rows == 0 || P == ix->tk_dim, "%s: the queries have P=%d, the stored matrices P=%d", fn, P, ix->tk_dim);
    rc = hc.upload(allow_bits_host, ix->tk_bq, (const uint32_t*)in.data(), in.size(), (size_t)nq * k);
    if (rc == CSS_OK) {
        const hipStream_t st = ix->stream;
        const Rows& rows = hc.rows;
        const unsigned short* q_dev = reinterpret_cast<const unsigned short*>(ix->tk_bq.p + at);
        const int64_t *qoff_dev = reinterpret_cast<const int64_t*>(ix->tk_bq.p), *qoff = q_offsets_host;
        WsTurn turn(ix, st);
        if ((rc = turn.rc) == CSS_OK) {
            ix->last_maxsim_passes = 0;
            // per group of kTokGroup queries ONE pass over the store; a group of one runs the single call's kernel
            rc = tok_topk_enqueue(ix, ix->lex_col, rows.n, rows.mask, rows.id_base, nq, kTokGroup, k, hc.d_out, hc.i_out, fn, st,
                                  [&](int q0, int ng, float* col) {
                                      int mq_max = 0;
                                      for (int b = q0; b < q0 + ng; ++b) mq_max = std::max(mq_max, (int)(qoff[b + 1] - qoff[b]));
                                      const int rc = ng == 1 ? tok_scores_enqueue(ix, nullptr, rows.n, rows.mask,
                                                                                  q_dev + (size_t)qoff[q0] * P, mq_max, col, st)
                                                             : tok_scores_group_enqueue(ix, rows.n, rows.mask, q_dev, qoff_dev + q0, ng,
                                                                                        mq_max, col, st);
                                      if (rc == CSS_OK) ++ix->last_maxsim_passes;
                                      return rc;
                                  });
        }
    }
    return hc.finish(rc, D_host, I_host);
}

int css_index_last_maxsim_passes(css_index* ix, int* passes_out) {
    CSS_REQUIRE(ix && passes_out, "css_index_last_maxsim_passes: NULL argument");
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    *passes_out = ix->last_maxsim_passes;
    return CSS_OK;
}

int css_index_maxsim_rows(css_index* ix, const uint16_t* q_tok_host, int mq, int P, const int64_t* ids_host, int64_t n,
                          float* scores_out) {
    CSS_REQUIRE(ix, "css_index_maxsim_rows: NULL index");
    CSS_REQUIRE(n >= 0 && n <= CSS_MAX_MAXSIM_ROWS, "css_index_maxsim_rows: n=%lld outside [0, %d]", (long long)n, CSS_MAX_MAXSIM_ROWS);
    CSS_REQUIRE(n == 0 || (ids_host && scores_out), "css_index_maxsim_rows: NULL buffer");
    int rc = token_query_check("css_index_maxsim_rows", q_tok_host, mq, P);
    if (rc != CSS_OK) return rc;
    CallScope cs(ix);
    CSS_REQUIRE(ix->tk_rows == 0 || P == ix->tk_dim, "css_index_maxsim_rows: the query has P=%d, the stored matrices P=%d", P,
                ix->tk_dim);
    for (int64_t i = 0; i < n; ++i)
        CSS_REQUIRE(ids_host[i] >= cs.rows.id_base && ids_host[i] - cs.rows.id_base < cs.rows.n,
                    "css_index_maxsim_rows: id %lld (position %lld) is outside the index's [%lld, %lld)", (long long)ids_host[i],
                    (long long)i, (long long)cs.rows.id_base, (long long)(cs.rows.id_base + cs.rows.n));
    if (n == 0) return CSS_OK;
    if (ix->tk_rows == 0) {   // no matrices: every row is a miss
        for (int64_t i = 0; i < n; ++i) scores_out[i] = -INFINITY;
        return CSS_OK;
    }
    // the ONE upload: [row numbers | the query matrix] (the matrix behind the 4-byte numbers: 16-byte aligned rows)
    const size_t nq_words = ((size_t)mq * P + 1) / 2, at = ((size_t)n + 3) / 4 * 4;
    std::vector<uint32_t> in;
    try {
        in.assign(at + nq_words, 0u);
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_maxsim_rows: out of host memory");
        return CSS_ERR_OOM;
    }
    for (int64_t i = 0; i < n; ++i) in[(size_t)i] = (uint32_t)(ids_host[i] - cs.rows.id_base);
    memcpy(in.data() + at, q_tok_host, (size_t)mq * P * sizeof(uint16_t));
    const hipStream_t st = ix->stream;
    if ((rc = ix->tk_ids.grow(in.size())) != CSS_OK) return rc;
    if ((rc = ix->tk_col.grow((size_t)n)) != CSS_OK) return rc;
    {
        WsTurn turn(ix, st);
        rc = turn.rc;
        if (rc == CSS_OK) {
            const hipError_t e = hipMemcpyAsync(ix->tk_ids.p, in.data(), in.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) rc = css::hip_fail(e, "hipMemcpyAsync(row numbers)", __FILE__, __LINE__);
        }
        if (rc == CSS_OK && ix->ingest_pending) {
            const hipError_t e = hipStreamWaitEvent(st, ix->ingest_ev, 0);
            if (e != hipSuccess) rc = css::hip_fail(e, "hipStreamWaitEvent(ingest)", __FILE__, __LINE__);
        }
        if (rc == CSS_OK)
            rc = tok_scores_enqueue(ix, ix->tk_ids.p, n, nullptr, reinterpret_cast<const unsigned short*>(ix->tk_ids.p + at), mq,
                                    ix->tk_col.p, st);
        if (rc == CSS_OK) {
            const hipError_t e = hipMemcpyAsync(scores_out, ix->tk_col.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) rc = css::hip_fail(e, "hipMemcpyAsync(scores)", __FILE__, __LINE__);
        }
    }
    const hipError_t e = hipStreamSynchronize(st);   // (also after a failure: the copies read this call's memory)
    if (rc != CSS_OK) return rc;
    CSS_HIP_TRY(e);
    return CSS_OK;
}

// ------------------------------------------------------------------ MaxSim over per-query row lists, two-stage search
namespace {
// What both list entry points check of their queries before anything is enqueued (the store's P under the call's locks)
int token_batch_check(const char* fn, const uint16_t* q_tok_host, const int64_t* q_offsets_host, int nq, int P) {
    CSS_REQUIRE(nq >= 1 && nq <= CSS_MAX_MAXSIM_QUERIES, "%s: nq=%d outside [1, %d]", fn, nq, CSS_MAX_MAXSIM_QUERIES);
    CSS_REQUIRE(q_tok_host && q_offsets_host, "%s: NULL buffer", fn);
    CSS_REQUIRE(token_dim_ok(P), "%s: P=%d must be a multiple of 32 in [32, %d]", fn, P, CSS_MAX_TOKEN_DIM);
    CSS_REQUIRE(q_offsets_host[0] == 0, "%s: the offsets start at %lld, not at 0", fn, (long long)q_offsets_host[0]);
    int rc;
    for (int b = 0; b < nq; ++b)
        if ((rc = token_len_check(fn, q_offsets_host[b + 1] - q_offsets_host[b], b)) != CSS_OK) return rc;
    for (int b = 0; b < nq; ++b)
        if ((rc = token_finite_check(fn, q_tok_host + (size_t)q_offsets_host[b] * P, (int)(q_offsets_host[b + 1] - q_offsets_host[b]),
                                     P, b)) != CSS_OK) return rc;
    return CSS_OK;
}
int token_batch_longest(const int64_t* qoff, int nq) {
    int64_t m = 0;
    for (int b = 0; b < nq; ++b) m = std::max(m, qoff[b + 1] - qoff[b]);
    return (int)m;
}

// col[b][j] = the MaxSim of query b (tokens q, offsets qoff [nq + 1] on the device; mq_max: the longest) with row
// lists[b][j] (kTokNoRow: none), -inf for a miss: ONE launch.  The index has matrices.  Enqueued on `st`.
int tok_lists_enqueue(css_index* ix, const uint32_t* lists, int nq, int f, const unsigned short* q, const int64_t* qoff,
                      int mq_max, float* col, hipStream_t st) {
    const void* fn = tok_variant(ix->tk_dim, (mq_max + 15) / 16, ix->tk_bits, [](auto p, auto mt, auto nb) {
        return (const void*)k_tok_scores_l<decltype(p)::value, decltype(mt)::value, decltype(nb)::value>;
    });
    int rc, per;
    unsigned grid;
    if ((rc = tok_grid(ix, fn, 64 * kWaves, (int64_t)nq * f, kWaves, &per, &grid)) != CSS_OK) return rc;
    TokStore store = tok_store(ix);
    void* args[] = {&store, &lists, &nq, &f, &q, &qoff, &per, &col};
    ProfScope ps(ix->tk_bits ? "tok_scores_lc" : "tok_scores_l", st);
    CSS_HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(64 * kWaves), args, 0, st));
    return CSS_OK;
}

// The pool search (search_any_k: every mode, shadow policy and mask as css_index_search_masked has them) into the owned
// pool lists, the lists as row numbers under `floor`, their MaxSim with the queries' matrices in one launch, the k best
// POSITIONS of each list and the four outputs.  Everything is enqueued on `st`; nothing waits for the device.  Caller
// holds ws_mu and a shared lock on mu.
int search_rerank_enqueue(css_index* ix, const Rows& rows, const float* q_dev, int nq, int normalize_q,
                          const unsigned short* tok_dev, const int64_t* qoff_dev, int mq_max, int fetch, int k, float floor,
                          float* D_dev, int64_t* I_dev, float* S_dev, int32_t* R_dev, hipStream_t st) {
    int rc;
    const int64_t total = (int64_t)nq * k, pool = (int64_t)nq * fetch;
    WsTurn turn(ix, st);   // (until the end: every kernel behind the search reads the pool lists)
    if (turn.rc != CSS_OK) return turn.rc;
    if (ix->tk_rows == 0) {   // no matrices: every pool entry is a miss
        hipLaunchKernelGGL(k_rr_pad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, D_dev, I_dev, S_dev, R_dev);
        CSS_LAUNCH_CHECK();
        return CSS_OK;
    }
    CSS_REQUIRE(rows.n < 0xFFFFFFFFll, "css_index_search_rerank_maxsim: %lld rows exceed the 32-bit row numbers of the lists",
                (long long)rows.n);
    // rows appended on another stream must have landed (an empty pool search does not wait for them itself)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->rr_d.grow((size_t)pool)) != CSS_OK) return rc;
    if ((rc = ix->rr_i.grow((size_t)pool)) != CSS_OK) return rc;
    if ((rc = ix->rr_rows.grow((size_t)pool)) != CSS_OK) return rc;
    if ((rc = ix->rr_col.grow((size_t)pool)) != CSS_OK) return rc;
    if ((rc = ix->sp_pd.grow((size_t)total)) != CSS_OK) return rc;
    if ((rc = ix->sp_pi.grow((size_t)total)) != CSS_OK) return rc;
    if ((rc = search_any_k(ix, rows, q_dev, nq, fetch, normalize_q, ix->rr_d.p, ix->rr_i.p, st)) != CSS_OK) return rc;
    {
        ProfScope ps("rr_lists", st);
        hipLaunchKernelGGL(k_rr_lists, dim3((unsigned)((pool + 255) / 256)), dim3(256), 0, st, (const int64_t*)ix->rr_i.p,
                           (const float*)ix->rr_d.p, pool, rows.id_base, floor, ix->rr_rows.p);
        CSS_LAUNCH_CHECK();
    }
    if ((rc = tok_lists_enqueue(ix, ix->rr_rows.p, nq, fetch, tok_dev, qoff_dev, mq_max, ix->rr_col.p, st)) != CSS_OK) return rc;
    {
        // one slice per list (no part merge), positions in place of ids: ties go to the lower POSITION
        ProfScope ps("rr_topk", st);
        hipLaunchKernelGGL(k_sparse_topk_cols, dim3(1, (unsigned)nq), dim3(256), 0, st, (const float*)ix->rr_col.p, (int64_t)fetch,
                           (int64_t)fetch, (const uint32_t*)nullptr, k, (int64_t)0, ix->sp_pd.p, ix->sp_pi.p);
        CSS_LAUNCH_CHECK();
    }
    ProfScope ps("rr_out", st);
    hipLaunchKernelGGL(k_rr_out, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)ix->sp_pd.p,
                       (const int64_t*)ix->sp_pi.p, (const float*)ix->rr_d.p, (const int64_t*)ix->rr_i.p, fetch, k, total, D_dev,
                       I_dev, S_dev, R_dev);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}
}  // namespace

int css_index_maxsim_rows_batch(css_index* ix, const uint16_t* q_tok_host, const int64_t* q_offsets_host, int nq, int P,
                                const int64_t* ids_host, int f, float* scores_out) {
    const char* fn = "css_index_maxsim_rows_batch";
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    int rc = token_batch_check(fn, q_tok_host, q_offsets_host, nq, P);
    if (rc != CSS_OK) return rc;
    CSS_REQUIRE(f >= 1 && f <= CSS_MAX_K, "%s: f=%d outside [1, %d]", fn, f, CSS_MAX_K);
    CSS_REQUIRE(ids_host && scores_out, "%s: NULL buffer", fn);
    CallScope cs(ix);
    CSS_REQUIRE(ix->tk_rows == 0 || P == ix->tk_dim, "%s: the queries have P=%d, the stored matrices P=%d", fn, P, ix->tk_dim);
    const size_t total = (size_t)nq * f;
    if (ix->tk_rows == 0) {   // no matrices: every row is a miss
        for (size_t i = 0; i < total; ++i) scores_out[i] = -INFINITY;
        return CSS_OK;
    }
    CSS_REQUIRE(cs.rows.n < 0xFFFFFFFFll, "%s: %lld rows exceed the 32-bit row numbers of the lists", fn, (long long)cs.rows.n);
    // the ONE upload: [offsets (int64) | row numbers | the matrices], each part at a multiple of 16 bytes
    const size_t ntok = (size_t)q_offsets_host[nq];
    const size_t at_ids = ((size_t)(nq + 1) * 2 + 3) / 4 * 4, at_tok = at_ids + (total + 3) / 4 * 4, q_words = ntok * P / 2;
    std::vector<uint32_t> in;
    try {
        in.assign(at_tok + q_words, 0u);
    } catch (const std::bad_alloc&) {
        css::set_error("%s: out of host memory", fn);
        return CSS_ERR_OOM;
    }
    memcpy(in.data(), q_offsets_host, (size_t)(nq + 1) * sizeof(int64_t));
    for (size_t i = 0; i < total; ++i) {   // an id outside the index names no row
        const int64_t r = ids_host[i] - cs.rows.id_base;
        in[at_ids + i] = (ids_host[i] >= cs.rows.id_base && r < cs.rows.n) ? (uint32_t)r : kTokNoRow;
    }
    memcpy(in.data() + at_tok, q_tok_host, ntok * P * sizeof(uint16_t));
    const hipStream_t st = ix->stream;
    if ((rc = ix->tk_bq.grow(in.size())) != CSS_OK) return rc;
    if ((rc = ix->tk_col.grow(total)) != CSS_OK) return rc;
    {
        WsTurn turn(ix, st);
        rc = turn.rc;
        if (rc == CSS_OK) {
            const hipError_t e = hipMemcpyAsync(ix->tk_bq.p, in.data(), in.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) rc = css::hip_fail(e, "hipMemcpyAsync(lists)", __FILE__, __LINE__);
        }
        if (rc == CSS_OK && ix->ingest_pending) {
            const hipError_t e = hipStreamWaitEvent(st, ix->ingest_ev, 0);
            if (e != hipSuccess) rc = css::hip_fail(e, "hipStreamWaitEvent(ingest)", __FILE__, __LINE__);
        }
        if (rc == CSS_OK)
            rc = tok_lists_enqueue(ix, ix->tk_bq.p + at_ids, nq, f, reinterpret_cast<const unsigned short*>(ix->tk_bq.p + at_tok),
                                   reinterpret_cast<const int64_t*>(ix->tk_bq.p), token_batch_longest(q_offsets_host, nq),
                                   ix->tk_col.p, st);
        if (rc == CSS_OK) {
            const hipError_t e = hipMemcpyAsync(scores_out, ix->tk_col.p, total * sizeof(float), hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) rc = css::hip_fail(e, "hipMemcpyAsync(scores)", __FILE__, __LINE__);
        }
    }
    const hipError_t e = hipStreamSynchronize(st);   // (also after a failure: the copies read this call's memory)
    if (rc != CSS_OK) return rc;
    CSS_HIP_TRY(e);
    return CSS_OK;
}

int css_index_search_rerank_maxsim(css_index* ix, const float* q_host, int normalize_q, const uint16_t* q_tok_host,
                                   const int64_t* q_offsets_host, int nq, int P, int fetch, int k, float floor,
                                   const uint32_t* allow_bits_host, float* D_host, int64_t* I_host, float* S_host, int32_t* R_host) {
    const char* fn = "css_index_search_rerank_maxsim";
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    int rc = token_batch_check(fn, q_tok_host, q_offsets_host, nq, P);
    if (rc != CSS_OK) return rc;
    CSS_REQUIRE(fetch >= 1 && fetch <= CSS_MAX_K, "%s: fetch=%d outside [1, %d]", fn, fetch, CSS_MAX_K);
    CSS_REQUIRE(k >= 1 && k <= std::min(fetch, CSS_KERNEL_MAX_K), "%s: k=%d outside [1, min(fetch=%d, %d)]", fn, k, fetch,
                CSS_KERNEL_MAX_K);
    CSS_REQUIRE(q_host && D_host && I_host && S_host && R_host, "%s: NULL buffer", fn);
    // the ONE upload: [dense queries (fp32) | offsets (int64) | the matrices], each part at a multiple of 16 bytes
    const size_t ntok = (size_t)q_offsets_host[nq], n = (size_t)nq * k;
    const size_t at_off = ((size_t)nq * ix->dim + 3) / 4 * 4, at_tok = at_off + ((size_t)(nq + 1) * 2 + 3) / 4 * 4;
    std::vector<uint32_t> in;
    std::vector<int32_t> sr;
    try {
        in.assign(at_tok + ntok * P / 2, 0u);
        sr.assign(2 * n, 0);
    } catch (const std::bad_alloc&) {
        css::set_error("%s: out of host memory", fn);
        return CSS_ERR_OOM;
    }
    memcpy(in.data(), q_host, (size_t)nq * ix->dim * sizeof(float));
    memcpy(in.data() + at_off, q_offsets_host, (size_t)(nq + 1) * sizeof(int64_t));
    memcpy(in.data() + at_tok, q_tok_host, ntok * P * sizeof(uint16_t));
    HostCall hc(ix);
    CSS_REQUIRE(ix->tk_rows == 0 || P == ix->tk_dim, "%s: the queries have P=%d, the stored matrices P=%d", fn, P, ix->tk_dim);
    hc.cols = 2;   // [S | R]
    rc = hc.upload(allow_bits_host, ix->rr_in, (const uint32_t*)in.data(), in.size(), n, &ix->rr_sr);
    if (rc == CSS_OK)
        rc = search_rerank_enqueue(ix, hc.rows, reinterpret_cast<const float*>(ix->rr_in.p), nq, normalize_q,
                                   reinterpret_cast<const unsigned short*>(ix->rr_in.p + at_tok),
                                   reinterpret_cast<const int64_t*>(ix->rr_in.p + at_off), token_batch_longest(q_offsets_host, nq),
                                   fetch, k, floor, hc.d_out, hc.i_out, reinterpret_cast<float*>(hc.g_out), hc.g_out + n, ix->stream);
    rc = hc.finish(rc, D_host, I_host, sr.data());
    if (rc != CSS_OK) return rc;
    memcpy(S_host, sr.data(), n * sizeof(float));
    memcpy(R_host, sr.data() + n, n * sizeof(int32_t));
    return CSS_OK;
}

namespace {
// The candidates of the query (mq tokens on the device) among `rows`: the centroid table, the approximate column over
// every row (lex_col), and the select of the best nc <= rows.n of it into tk_cand (ascending rows, 0xFFFFFFFF behind
// the count) and tk_capx; the count is word kSelHist + 3 of tk_sel.  The index has a codec and matrices, rows.n > 0.
// Everything is enqueued on `st`.  Caller holds ws_mu, a shared lock on mu and a turn at the workspaces.
int tok_candidates_enqueue(css_index* ix, const Rows& rows, const unsigned short* q_dev, int mq, int64_t nc, const char* who,
                           hipStream_t st) {
    int rc;
    CSS_REQUIRE(rows.n < 0xFFFFFFFFll, "%s: %lld rows exceed the 32-bit row numbers of the lists", who, (long long)rows.n);
    const int P = ix->tk_dim, MT = (mq + 15) / 16, W = 16 * MT, C = ix->tk_ncent;
    const int64_t n = rows.n;
    const int nblk = (int)((n + kSelSlice - 1) / kSelSlice);
    if ((rc = ix->tk_ctab.grow((size_t)C * W)) != CSS_OK) return rc;
    if ((rc = ix->lex_col.grow((size_t)n)) != CSS_OK) return rc;
    if ((rc = ix->tk_cand.grow((size_t)nc)) != CSS_OK) return rc;
    if ((rc = ix->tk_capx.grow((size_t)nc)) != CSS_OK) return rc;
    if ((rc = ix->tk_sel.grow((size_t)kSelState + 2 * (size_t)nblk)) != CSS_OK) return rc;
    // rows appended on another stream must have landed (the mask and the row count speak of them)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    const unsigned short* cent = ix->tk_cent.p;
    float* tab = ix->tk_ctab.p;
    {
        const void* fn = tok_dim(P, [](auto p) { return (const void*)k_tok_ctable<decltype(p)::value>; });
        int mt = MT, c = C, m = mq;
        void* args[] = {&cent, &c, &q_dev, &m, &mt, &tab};
        ProfScope ps("tok_ctable", st);
        CSS_HIP_TRY(hipLaunchKernel(fn, dim3((unsigned)((C + 16 * kWaves - 1) / (16 * kWaves))), dim3(64 * kWaves), args, 0, st));
    }
    {
        const void* fn = W <= 16 ? (const void*)k_tok_ci<16> : W <= 32 ? (const void*)k_tok_ci<32> : (const void*)k_tok_ci<64>;
        int per;
        unsigned grid;
        if ((rc = tok_grid(ix, fn, 64 * kWaves, n, kWaves, &per, &grid)) != CSS_OK) return rc;
        TokStore store = tok_store(ix);
        const float* ctab = tab;
        int64_t nn = n;
        const uint32_t *list = nullptr, *mask = rows.mask;
        int w = W, m = mq;
        float* col = ix->lex_col.p;
        void* args[] = {&store, &ctab, &w, &list, &nn, &mask, &m, &per, &col};
        ProfScope ps("tok_ci", st);
        CSS_HIP_TRY(hipLaunchKernel(fn, dim3(grid), dim3(64 * kWaves), args, 0, st));
    }
    ProfScope ps("tok_select", st);
    uint32_t* sel = ix->tk_sel.p;
    CSS_HIP_TRY(hipMemsetAsync(sel, 0, (size_t)kSelState * sizeof(uint32_t), st));
    CSS_HIP_TRY(hipMemsetAsync(ix->tk_cand.p, 0xFF, (size_t)nc * sizeof(uint32_t), st));
    const unsigned hblk = (unsigned)std::min(nblk, kSelMaxBlocks);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(k_sel_hist, dim3(hblk), dim3(256), 0, st, (const float*)ix->lex_col.p, n, (uint32_t)nc, pass, sel);
        CSS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_sel_count, dim3((unsigned)nblk), dim3(256), 0, st, (const float*)ix->lex_col.p, n, (uint32_t)nc,
                       (const uint32_t*)sel, sel + kSelHist, sel + kSelState);
    CSS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sel_write, dim3((unsigned)nblk), dim3(256), 0, st, (const float*)ix->lex_col.p, n,
                       (const uint32_t*)(sel + kSelState), nblk, (uint32_t)nc, sel + kSelHist, ix->tk_cand.p, ix->tk_capx.p);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// what both entry points check of the call before anything is enqueued; under the call's locks
int token_prune_check(const char* fn, const css_index* ix, int P, int64_t ncand) {
    CSS_REQUIRE(ix->tk_bits != 0, "%s: the index has no token codec (css_index_set_token_codec)", fn);
    CSS_REQUIRE(P == ix->tk_cdim, "%s: the query has P=%d, the index's token codec P=%d", fn, P, ix->tk_cdim);
    CSS_REQUIRE(ncand >= 1 && ncand <= CSS_MAX_MAXSIM_ROWS, "%s: ncand=%lld outside [1, %d]", fn, (long long)ncand, CSS_MAX_MAXSIM_ROWS);
    return CSS_OK;
}
}  // namespace

int css_index_maxsim_candidates(css_index* ix, const uint16_t* q_tok_host, int mq, int P, int64_t ncand,
                                const uint32_t* allow_bits_host, int64_t* ids_out, float* approx_out, int64_t* n_out) {
    const char* fn = "css_index_maxsim_candidates";
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    CSS_REQUIRE(ids_out && approx_out && n_out, "%s: NULL buffer", fn);
    int rc = token_query_check(fn, q_tok_host, mq, P);
    if (rc != CSS_OK) return rc;
    HostCall hc(ix);
    if ((rc = token_prune_check(fn, ix, P, ncand)) != CSS_OK) return rc;
    *n_out = 0;
    if (ix->tk_rows == 0 || hc.rows.n == 0) return CSS_OK;   // a codec without matrices: no candidates
    const int64_t nc = std::min<int64_t>(ncand, hc.rows.n);
    std::vector<float> Dh;
    std::vector<int64_t> Ih;
    try {
        Dh.resize((size_t)nc + 1);
        Ih.resize((size_t)nc + 1);
    } catch (const std::bad_alloc&) {
        css::set_error("%s: out of host memory", fn);
        return CSS_ERR_OOM;
    }
    // the ONE upload: the query matrix; the results: nc [id | approximate score] entries and the count behind them
    rc = hc.upload(allow_bits_host, ix->tk_q, (const unsigned short*)q_tok_host, (size_t)mq * P, (size_t)nc + 1);
    if (rc == CSS_OK) {
        const hipStream_t st = ix->stream;
        WsTurn turn(ix, st);
        rc = turn.rc;
        if (rc == CSS_OK) rc = tok_candidates_enqueue(ix, hc.rows, ix->tk_q.p, mq, nc, fn, st);
        if (rc == CSS_OK) {
            hipLaunchKernelGGL(k_tok_cand_out, dim3((unsigned)((nc + 256) / 256)), dim3(256), 0, st, (const uint32_t*)ix->tk_cand.p,
                               (const float*)ix->tk_capx.p, (const uint32_t*)(ix->tk_sel.p + kSelHist), nc, hc.rows.id_base,
                               hc.d_out, hc.i_out);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) rc = css::hip_fail(e, "k_tok_cand_out", __FILE__, __LINE__);
        }
    }
    if ((rc = hc.finish(rc, Dh.data(), Ih.data())) != CSS_OK) return rc;
    const int64_t got = Ih[(size_t)nc];
    memcpy(ids_out, Ih.data(), (size_t)got * sizeof(int64_t));
    memcpy(approx_out, Dh.data(), (size_t)got * sizeof(float));
    *n_out = got;
    return CSS_OK;
}

int css_index_search_maxsim_pruned(css_index* ix, const uint16_t* q_tok_host, int mq, int P, int k, int64_t ncand,
                                   const uint32_t* allow_bits_host, float* D_host, int64_t* I_host, int64_t* ncand_out) {
    const char* fn = "css_index_search_maxsim_pruned";
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    CSS_REQUIRE(k >= 1 && k <= CSS_KERNEL_MAX_K, "%s: k=%d outside [1, %d]", fn, k, CSS_KERNEL_MAX_K);
    CSS_REQUIRE(D_host && I_host, "%s: NULL buffer", fn);
    int rc = token_query_check(fn, q_tok_host, mq, P);
    if (rc != CSS_OK) return rc;
    HostCall hc(ix);
    if ((rc = token_prune_check(fn, ix, P, ncand)) != CSS_OK) return rc;
    CSS_REQUIRE(k <= ncand, "%s: k=%d exceeds ncand=%lld", fn, k, (long long)ncand);
    float Dh[CSS_KERNEL_MAX_K + 1];
    int64_t Ih[CSS_KERNEL_MAX_K + 1];
    // the ONE upload: the query matrix; the results: k entries and the candidate count in the id slot behind them
    rc = hc.upload(allow_bits_host, ix->tk_q, (const unsigned short*)q_tok_host, (size_t)mq * P, (size_t)k + 1);
    if (rc == CSS_OK) {
        const hipStream_t st = ix->stream;
        WsTurn turn(ix, st);
        rc = turn.rc;
        if (rc == CSS_OK) rc = [&]() -> int {
            int rc;
            if (ix->tk_rows == 0 || hc.rows.n == 0) {   // a codec without matrices: the padded answer, no candidates
                hipLaunchKernelGGL(k_sparse_pad, dim3(1), dim3(128), 0, st, hc.d_out, hc.i_out, k);
                CSS_LAUNCH_CHECK();
                CSS_HIP_TRY(hipMemsetAsync(hc.i_out + k, 0, sizeof(int64_t), st));
                return CSS_OK;
            }
            const int64_t nc = std::min<int64_t>(ncand, hc.rows.n);
            if ((rc = tok_candidates_enqueue(ix, hc.rows, ix->tk_q.p, mq, nc, fn, st)) != CSS_OK) return rc;
            // the exact scores of the candidates on the codes (a slot behind the count names no row: a miss) and their
            // top-k by (score, position): the list ascends by row, so ties go to the lower id ...
            if ((rc = tok_topk_enqueue(ix, ix->tk_col, nc, nullptr, 0, 1, 1, k, hc.d_out, hc.i_out, fn, st, [&](int, int, float* col) {
                    return tok_scores_enqueue(ix, ix->tk_cand.p, nc, nullptr, ix->tk_q.p, mq, col, st);
                })) != CSS_OK) return rc;
            // ... and the positions become ids
            hipLaunchKernelGGL(k_tok_cand_ids, dim3(1), dim3(256), 0, st, (const uint32_t*)ix->tk_cand.p,
                               (const uint32_t*)(ix->tk_sel.p + kSelHist), k, hc.rows.id_base, hc.d_out, hc.i_out);
            CSS_LAUNCH_CHECK();
            return CSS_OK;
        }();
    }
    if ((rc = hc.finish(rc, Dh, Ih)) != CSS_OK) return rc;
    memcpy(D_host, Dh, (size_t)k * sizeof(float));
    memcpy(I_host, Ih, (size_t)k * sizeof(int64_t));
    if (ncand_out) *ncand_out = Ih[k];
    return CSS_OK;
}

int css_merge_topk_dev(const float* Dp, const int64_t* Ip, int nparts, int64_t nq, int k, int metric, float* D,
                       int64_t* I, int device, void* stream) {
    return merge_parts(Dp, Ip, nparts, nq * k, nq * k, nq, k, metric, D, I, device, stream, "css_merge_topk_dev");
}

int css_merge_topk_packed_dev(const void* packed, int nparts, int64_t record_bytes, int64_t nq, int k, int metric,
                              float* D, int64_t* I, int device, void* stream) {
    CSS_REQUIRE(packed != nullptr, "css_merge_topk_packed_dev: NULL buffer");
    CSS_REQUIRE(nq >= 0 && k >= 1 && record_bytes >= 12 * nq * k && record_bytes % 8 == 0,
                "css_merge_topk_packed_dev: record of %lld bytes cannot hold [%lld x %d] ids and scores (multiple of 8)",
                (long long)record_bytes, (long long)nq, k);
    const int64_t* Ip = reinterpret_cast<const int64_t*>(packed);
    const float* Dp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(packed) + 8 * nq * k);
    return merge_parts(Dp, Ip, nparts, record_bytes / 4, record_bytes / 8, nq, k, metric, D, I, device, stream,
                       "css_merge_topk_packed_dev");
}

// ------------------------------------------------------------------ range search (variable-length results)
struct css_range_result {
    int64_t nq = 0;
    std::vector<int64_t> lims;   // nq + 1
    std::vector<float> D;
    std::vector<int64_t> I;
};

namespace {
// nq > 0 queries over hc.rows.n > 0 rows, inside the caller's host frame: the turn at the workspaces first, then the
// frame's upload of bitmap and queries (into q_raw; no result rows: `res` is filled here).  Everything runs on the
// index's own stream and has finished when this returns CSS_OK.
int range_search_locked(css_index* ix, HostCall& hc, const float* q_host, const uint32_t* allow_bits_host, int64_t nq,
                        float radius, int normalize_q, css_range_result* res) {
    hipStream_t st = ix->stream;
    int rc;
    CSS_REQUIRE(hc.rows.n < 0xFFFFFFFFll, "css_index_range_search: %lld rows exceed the 32-bit row numbers of the hit pool",
                (long long)hc.rows.n);
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if ((rc = hc.upload(allow_bits_host, ix->q_raw, q_host, (size_t)nq * ix->dim)) != CSS_OK) return rc;
    const Rows& rows = hc.rows;
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->qpad.grow((size_t)(nq + 256) * ix->dpad)) != CSS_OK) return rc;
    if ((rc = ix->qnorm2.grow((size_t)nq + 256)) != CSS_OK) return rc;
    if ((rc = ix->range_cnt.grow_exact(kRangeSlots, "hipMalloc(range counters)")) != CSS_OK) return rc;
    if (ix->range_cap() == 0 && range_pool_alloc(ix, kRangeInitialCap) != CSS_OK) {
        css::set_error("css_index_range_search: no device memory for the initial hit pool");
        return CSS_ERR_OOM;
    }
    if ((rc = prep_queries(ix, ix->q_raw.p, nq, normalize_q, nullptr, st)) != CSS_OK) return rc;
    const int nq_sweep = range_nq_sweep(ix);
    const bool ip = ix->metric == CSS_METRIC_IP;
    std::vector<float> hs;
    std::vector<uint32_t> hi;
    std::vector<uint32_t> order;
    unsigned int cnt[kRangeSlots];
    for (int64_t q0 = 0; q0 < nq; q0 += nq_sweep) {
        const int nqc = (int)std::min<int64_t>(nq_sweep, nq - q0);
        const float* qp = ix->qpad.p + (size_t)q0 * ix->dpad;
        if ((rc = range_sweep(ix, rows, qp, nqc, radius, cnt, st)) != CSS_OK) return rc;
        size_t most = 0, total = 0;
        for (int j = 0; j < nqc; ++j) {
            most = std::max<size_t>(most, cnt[j]);
            total += cnt[j];
        }
        if (most > ix->range_cap()) {
            // the sweep counted every hit: grow to that size and sweep ONCE more (never a loop)
            if (range_pool_alloc(ix, most) != CSS_OK) {
                css::set_error("css_index_range_search: no device memory for the hit pool: %zu hits for one query "
                               "(%zu for %d queries of the batch)", most, total, nqc);
                return CSS_ERR_OOM;
            }
            if ((rc = range_sweep(ix, rows, qp, nqc, radius, cnt, st)) != CSS_OK) return rc;
            for (int j = 0; j < nqc; ++j)
                if (cnt[j] > ix->range_cap()) {   // (rows and mask cannot change under the locks held)
                    css::set_error("css_index_range_search: internal: the second sweep counted more hits than the first");
                    return CSS_ERR_STATE;
                }
            total = 0;
            for (int j = 0; j < nqc; ++j) total += cnt[j];
        }
        try {
            res->D.reserve(res->D.size() + total);
            res->I.reserve(res->I.size() + total);
            for (int j = 0; j < nqc; ++j) {
                const size_t c = cnt[j];
                hs.resize(c);
                hi.resize(c);
                order.resize(c);
                if (c) {
                    CSS_HIP_TRY(hipMemcpyAsync(hs.data(), ix->range_s.p + (size_t)j * ix->range_cap(), c * sizeof(float), hipMemcpyDeviceToHost, st));
                    CSS_HIP_TRY(hipMemcpyAsync(hi.data(), ix->range_i.p + (size_t)j * ix->range_cap(), c * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    CSS_HIP_TRY(hipStreamSynchronize(st));
                }
                // the defined order, formed here on the host: best score first, equal scores by ascending id
                for (size_t i = 0; i < c; ++i) order[i] = (uint32_t)i;
                std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                    if (hs[a] != hs[b]) return ip ? hs[a] > hs[b] : hs[a] < hs[b];
                    return hi[a] < hi[b];
                });
                for (size_t i = 0; i < c; ++i) {
                    res->D.push_back(hs[order[i]]);
                    res->I.push_back(rows.id_base + (int64_t)hi[order[i]]);
                }
                res->lims[(size_t)(q0 + j + 1)] = (int64_t)res->D.size();
            }
        } catch (const std::bad_alloc&) {
            css::set_error("css_index_range_search: no host memory for %zu hits of %d queries", total, nqc);
            return CSS_ERR_OOM;
        }
    }
    return CSS_OK;
}
}  // namespace

int css_index_range_search(css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q,
                           const uint32_t* allow_bits_host, css_range_result** out) {
    CSS_REQUIRE(ix, "css_index_range_search: NULL index");
    CSS_REQUIRE(out, "css_index_range_search: out is NULL");
    *out = nullptr;
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "css_index_range_search: nq=%lld out of range", (long long)nq);
    CSS_REQUIRE(!std::isnan(radius), "css_index_range_search: the radius is NaN");
    CSS_REQUIRE(nq == 0 || q_host, "css_index_range_search: NULL buffer");
    css_range_result* res = new (std::nothrow) css_range_result();
    if (res) {
        try {
            res->lims.assign((size_t)nq + 1, 0);
            res->nq = nq;
        } catch (const std::bad_alloc&) {
            delete res;
            res = nullptr;
        }
    }
    if (!res) {
        css::set_error("css_index_range_search: no host memory for the result of %lld queries", (long long)nq);
        return CSS_ERR_OOM;
    }
    int rc = CSS_OK;
    if (nq > 0) {   // (an empty index or no query touches no device)
        HostCall hc(ix, nullptr, false);
        if (hc.rows.n > 0)
            rc = hc.wait_if_failed(range_search_locked(ix, hc, q_host, allow_bits_host, nq, radius, normalize_q, res));
    }
    if (rc != CSS_OK) {
        delete res;
        return rc;
    }
    *out = res;
    return CSS_OK;
}

// ------------------------------------------------------------------ facet counts
namespace {
// nq > 0 queries over hc.rows.n > 0 rows inside the caller's host frame, the outputs already at their empty values:
// the turn at the workspaces, the frame's upload of bitmap and queries, the bucket column, then one table per sweep
// decoded into the caller's arrays.  Everything has finished on the index's own stream when this returns CSS_OK.
// bucket_col: a device column of the index in the place of buckets_host / the labels (css_index_facets_attr).
int facets_locked(css_index* ix, HostCall& hc, const float* q_host, const uint32_t* allow_bits_host, int64_t nq, float radius,
                  int normalize_q, const int32_t* buckets_host, int64_t nbuckets, int64_t* count_out, float* best_score_out,
                  int64_t* best_id_out, int64_t* total_out, int64_t* unbucketed_out, const int32_t* bucket_col = nullptr) {
    hipStream_t st = ix->stream;
    int rc;
    CSS_REQUIRE(hc.rows.n < 0xFFFFFFFFll, "css_index_facets: %lld rows exceed the 32-bit row numbers of the table keys",
                (long long)hc.rows.n);
    const int nq_sweep = (int)std::min<int64_t>(range_nq_sweep(ix), std::max<int64_t>(1, kFacetMaxEntries / nbuckets));
    const size_t words = facet_tab_words((size_t)std::min<int64_t>(nq_sweep, nq) * (size_t)nbuckets);
    std::vector<unsigned long long> tab;
    try {
        tab.resize(words);
    } catch (const std::bad_alloc&) {
        css::set_error("css_index_facets: no host memory for a table of %lld buckets", (long long)nbuckets);
        return CSS_ERR_OOM;
    }
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if ((rc = hc.upload(allow_bits_host, ix->q_raw, q_host, (size_t)nq * ix->dim)) != CSS_OK) return rc;
    const Rows& rows = hc.rows;
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    if ((rc = ix->qpad.grow((size_t)(nq + 256) * ix->dpad)) != CSS_OK) return rc;
    if ((rc = ix->qnorm2.grow((size_t)nq + 256)) != CSS_OK) return rc;
    if (!ix->facet_tab.try_exact(words)) {
        css::set_error("css_index_facets: no device memory for a table of %lld queries x %lld buckets",
                       (long long)std::min<int64_t>(nq_sweep, nq), (long long)nbuckets);
        return CSS_ERR_OOM;
    }
    // (null: no label was ever set, every hit is unbucketed; bucket_col: the attribute column of css_index_facets_attr)
    const int32_t* bucket = bucket_col ? bucket_col : rows.labels;
    if (buckets_host) {
        if (!ix->facet_col.try_exact((size_t)rows.n)) {
            css::set_error("css_index_facets: no device memory for the bucket column of %lld rows", (long long)rows.n);
            return CSS_ERR_OOM;
        }
        CSS_HIP_TRY(hipMemcpyAsync(ix->facet_col.p, buckets_host, (size_t)rows.n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        bucket = ix->facet_col.p;
    }
    if ((rc = prep_queries(ix, ix->q_raw.p, nq, normalize_q, nullptr, st)) != CSS_OK) return rc;
    const bool ip = ix->metric == CSS_METRIC_IP;
    for (int64_t q0 = 0; q0 < nq; q0 += nq_sweep) {
        const int nqc = (int)std::min<int64_t>(nq_sweep, nq - q0);
        const size_t E = (size_t)nqc * (size_t)nbuckets;
        bool lds = false;
        if ((rc = facet_sweep(ix, rows, ix->qpad.p + (size_t)q0 * ix->dpad, nqc, radius, bucket, (int)nbuckets, tab.data(), &lds,
                              st)) != CSS_OK)
            return rc;
        ++ix->last_facet_sweeps;
        ix->last_facet_lds_sweeps += lds ? 1 : 0;
        const unsigned int* w = reinterpret_cast<const unsigned int*>(tab.data() + E);
        for (int j = 0; j < nqc; ++j) {
            total_out[q0 + j] = (int64_t)w[j];
            unbucketed_out[q0 + j] = (int64_t)w[16 + j];
        }
        const size_t o0 = (size_t)q0 * (size_t)nbuckets;
        for (size_t e = 0; e < E; ++e) {
            const unsigned int c = w[32 + e];
            count_out[o0 + e] = (int64_t)c;
            if (c == 0) continue;
            const unsigned long long key = tab[e];
            uint32_t u = (uint32_t)(key >> 32);
            if (!ip) u = ~u;
            u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
            if (best_score_out) memcpy(best_score_out + o0 + e, &u, sizeof(float));
            if (best_id_out) best_id_out[o0 + e] = rows.id_base + (int64_t)(uint32_t)~(uint32_t)key;
        }
    }
    return CSS_OK;
}

// The two entry points: the buckets are buckets_host / the labels (slot < 0), or the int32 attribute column `slot`
int facets_call(const char* fn, css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q, const uint32_t* allow_bits_host,
                const int32_t* buckets_host, int slot, int64_t nbuckets, int64_t* count_out, float* best_score_out,
                int64_t* best_id_out, int64_t* total_out, int64_t* unbucketed_out) {
    CSS_REQUIRE(ix, "%s: NULL index", fn);
    CSS_REQUIRE(nq >= 0 && nq < (1 << 24), "%s: nq=%lld out of range", fn, (long long)nq);
    CSS_REQUIRE(!std::isnan(radius), "%s: the radius is NaN", fn);
    CSS_REQUIRE(nbuckets >= 1 && nbuckets <= CSS_MAX_FACET_BUCKETS, "%s: nbuckets=%lld outside [1, %d]", fn,
                (long long)nbuckets, CSS_MAX_FACET_BUCKETS);
    CSS_REQUIRE(nq == 0 || (q_host && count_out && total_out && unbucketed_out), "%s: NULL buffer", fn);
    if (nq == 0) return CSS_OK;   // (no query touches no device)
    HostCall hc(ix, nullptr, false);
    const int32_t* bucket_col = nullptr;
    if (slot >= 0) {   // (under the shared lock: the slot cannot change before the sweep has read it)
        CSS_REQUIRE(ix->attrs[slot].type == CSS_ATTR_I32, "css_index_facets_attr: attribute slot %d %s", slot,
                    ix->attrs[slot].type < 0 ? "was never set" : "is float32 (buckets are an int32 column)");
        bucket_col = ix->attrs[slot].words.p;
    }
    ix->last_facet_sweeps = ix->last_facet_lds_sweeps = 0;
    // the answer of an empty index, and the empty slots of any other
    const size_t n = (size_t)nq * (size_t)nbuckets;
    std::fill(count_out, count_out + n, (int64_t)0);
    if (best_score_out) std::fill(best_score_out, best_score_out + n, pad_score(ix));
    if (best_id_out) std::fill(best_id_out, best_id_out + n, (int64_t)-1);
    std::fill(total_out, total_out + nq, (int64_t)0);
    std::fill(unbucketed_out, unbucketed_out + nq, (int64_t)0);
    if (hc.rows.n == 0) return CSS_OK;
    return hc.wait_if_failed(facets_locked(ix, hc, q_host, allow_bits_host, nq, radius, normalize_q, buckets_host, nbuckets,
                                           count_out, best_score_out, best_id_out, total_out, unbucketed_out, bucket_col));
}
}  // namespace

int css_index_facets(css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q,
                     const uint32_t* allow_bits_host, const int32_t* buckets_host, int64_t nbuckets, int64_t* count_out,
                     float* best_score_out, int64_t* best_id_out, int64_t* total_out, int64_t* unbucketed_out) {
    return facets_call("css_index_facets", ix, q_host, nq, radius, normalize_q, allow_bits_host, buckets_host, -1, nbuckets, count_out,
                       best_score_out, best_id_out, total_out, unbucketed_out);
}

int css_index_facets_attr(css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q,
                          const uint32_t* allow_bits_host, int slot, int64_t nbuckets, int64_t* count_out,
                          float* best_score_out, int64_t* best_id_out, int64_t* total_out, int64_t* unbucketed_out) {
    CSS_REQUIRE(slot >= 0 && slot < CSS_MAX_ATTRS, "css_index_facets_attr: attribute slot %d outside [0, %d)", slot,
                CSS_MAX_ATTRS);
    return facets_call("css_index_facets_attr", ix, q_host, nq, radius, normalize_q, allow_bits_host, nullptr, slot, nbuckets, count_out,
                       best_score_out, best_id_out, total_out, unbucketed_out);
}

int css_index_last_facet_sweeps(css_index* ix, int64_t* sweeps, int64_t* lds_sweeps) {
    CSS_REQUIRE(ix && sweeps && lds_sweeps, "css_index_last_facet_sweeps: NULL argument");
    std::lock_guard<std::mutex> wl(ix->ws_mu);
    *sweeps = ix->last_facet_sweeps;
    *lds_sweeps = ix->last_facet_lds_sweeps;
    return CSS_OK;
}

int css_index_set_facet_lds_entries(css_index* ix, int64_t entries) {
    CSS_REQUIRE(ix, "css_index_set_facet_lds_entries: NULL index");
    CSS_REQUIRE(entries >= -1, "css_index_set_facet_lds_entries: entries=%lld below -1", (long long)entries);
    std::unique_lock<std::shared_mutex> lk(ix->mu);
    ix->facet_lds_entries = entries;
    return CSS_OK;
}

int css_range_result_lims(const css_range_result* r, int64_t* lims_host) {
    CSS_REQUIRE(r && lims_host, "css_range_result_lims: NULL argument");
    memcpy(lims_host, r->lims.data(), r->lims.size() * sizeof(int64_t));
    return CSS_OK;
}

int css_range_result_read(const css_range_result* r, float* D_host, int64_t* I_host) {
    CSS_REQUIRE(r, "css_range_result_read: NULL result");
    if (r->D.empty()) return CSS_OK;
    CSS_REQUIRE(D_host && I_host, "css_range_result_read: NULL buffer");
    memcpy(D_host, r->D.data(), r->D.size() * sizeof(float));
    memcpy(I_host, r->I.data(), r->I.size() * sizeof(int64_t));
    return CSS_OK;
}

int css_range_result_free(css_range_result* r) {
    delete r;
    return CSS_OK;
}

// ------------------------------------------------------------------ rows by id, k-means step
int css_index_export_rows(css_index* ix, const int64_t* ids_host, int64_t n, float* x_out_host) {
    CSS_REQUIRE(ix, "css_index_export_rows: NULL index");
    CSS_REQUIRE(n >= 0 && n < (1 << 24), "css_index_export_rows: n=%lld out of range", (long long)n);
    if (n == 0) return CSS_OK;
    CSS_REQUIRE(ids_host && x_out_host, "css_index_export_rows: NULL buffer");
    HostCall hc(ix);
    const Rows& rows = hc.rows;   // (the id range check comes before anything is enqueued)
    for (int64_t j = 0; j < n; ++j)
        CSS_REQUIRE(ids_host[j] >= rows.id_base && ids_host[j] - rows.id_base < rows.n,
                    "css_index_export_rows: id %lld (entry %lld) outside [%lld, %lld)", (long long)ids_host[j], (long long)j,
                    (long long)rows.id_base, (long long)(rows.id_base + rows.n));
    const hipStream_t st = ix->stream;
    int rc = hc.upload(nullptr, ix->rowq_ids, ids_host, (size_t)n);
    if (rc == CSS_OK) rc = [&]() -> int {
        WsTurn turn(ix, st);
        if (turn.rc != CSS_OK) return turn.rc;
        if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
        int r;
        if ((r = ix->rowq.grow((size_t)n * ix->dim)) != CSS_OK) return r;
        if ((r = ix->rowq_flag.grow((size_t)n)) != CSS_OK) return r;
        hipLaunchKernelGGL(k_gather_queries, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, rows.xb,
                           (const int64_t*)ix->rowq_ids.p, ix->rowq.p, ix->rowq_flag.p, n, rows.n, rows.id_base, ix->dim, ix->dpad);
        CSS_LAUNCH_CHECK();
        CSS_HIP_TRY(hipMemcpyAsync(x_out_host, ix->rowq.p, (size_t)n * ix->dim * sizeof(float), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipStreamSynchronize(st));
        return CSS_OK;
    }();
    return hc.wait_if_failed(rc);
}

namespace {
// The centroid table, the assignment, the member lists and the sums of one Lloyd step (css_kmeans.h).  Everything is
// enqueued on `st`; nothing waits for the device.  Caller holds ws_mu and a shared lock on mu.
int kmeans_step_enqueue(css_index* ix, const Rows& rows, const float* craw_dev, int nc, int fx_shift, hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    // rows appended on another stream must have landed (their norms and the running maximum with them)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    const int nctiles = (nc + MF_BM - 1) / MF_BM, ncpad = nctiles * MF_BM;
    const size_t n1 = (size_t)std::max<int64_t>(rows.n, 1);
    if ((rc = ix->km_ctab.grow((size_t)ncpad * ix->dpad + ncpad)) != CSS_OK) return rc;
    if ((rc = ix->km_out.grow((size_t)KM_HDR + nc + (size_t)nc * ix->dim)) != CSS_OK) return rc;
    if ((rc = ix->km_off.grow((size_t)3 * nc + 2)) != CSS_OK) return rc;
    if ((rc = ix->km_assign.grow(n1)) != CSS_OK) return rc;
    if ((rc = ix->km_dist.grow(n1)) != CSS_OK) return rc;
    if ((rc = ix->km_members.grow(n1)) != CSS_OK) return rc;
    long long* hdr = ix->km_out.p;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(hdr + KM_HDR);
    unsigned long long* sums = counts + nc;
    uint32_t *off = ix->km_off.p, *seg = off + nc + 1, *cursor = seg + nc + 1;
    CSS_HIP_TRY(hipMemsetAsync(hdr, 0, ((size_t)KM_HDR + nc + (size_t)nc * ix->dim) * sizeof(long long), st));
    hipLaunchKernelGGL(k_kmeans_params, dim3(1), dim3(64), 0, st, (const int*)ix->maxn2.p, rows.n, fx_shift, hdr);
    CSS_LAUNCH_CHECK();
    if (rows.n == 0) return CSS_OK;   // zero sums and counts
    CSS_REQUIRE(rows.n < 0xFFFFFFFFll, "css_index_kmeans_step: %lld rows exceed the 32-bit row numbers of the member lists",
                (long long)rows.n);
    CSS_REQUIRE(ix->dpad % MF_BK == 0, "css_index_kmeans_step: internal: dpad=%d is no multiple of %d", ix->dpad, MF_BK);
    float* ctab = ix->km_ctab.p;
    float* cn2 = ctab + (size_t)ncpad * ix->dpad;
    // the table: the row kernel of ingest pads the centroids and forms ||c||^2 in fp32; pad centroids are zero rows
    // with ||c||^2 = +inf
    if (ncpad > nc) {
        CSS_HIP_TRY(hipMemsetAsync(ctab + (size_t)nc * ix->dpad, 0, (size_t)(ncpad - nc) * ix->dpad * sizeof(float), st));
        hipLaunchKernelGGL(k_fill_int, dim3(1), dim3(128), 0, st, reinterpret_cast<int*>(cn2 + nc), ncpad - nc, 0x7f800000);
        CSS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ingest_rows<false>, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, craw_dev, ctab, cn2, (int64_t)nc,
                       ix->dim, ix->dpad, 0, 0ull, 0ll, (unsigned short*)nullptr, (int*)nullptr, (float*)nullptr,
                       (unsigned char*)nullptr, (float*)nullptr);
    CSS_LAUNCH_CHECK();
    CSS_HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)nc * sizeof(uint32_t), st));
    {
        const int64_t ntiles = (rows.n + MF_BN - 1) / MF_BN;
        const int64_t want = std::min<int64_t>(ntiles, 2 * (int64_t)ix->num_cus);   // two blocks per CU
        const int64_t tpb = (ntiles + want - 1) / want;
        const unsigned grid = (unsigned)((ntiles + tpb - 1) / tpb);
        const size_t lds = (size_t)(2 * MF_BM * MF_BK + 2 * MF_BN * MF_BK + ncpad + nc) * 4;
        if ((rc = css::ensure_dynamic_lds((const void*)k_kmeans_assign, lds, ix->device)) != CSS_OK) return rc;
        ProfScope ps("kmeans_assign", st);
        hipLaunchKernelGGL(k_kmeans_assign, dim3(grid), dim3(256), lds, st, rows.xb, rows.xnorm2, (const float*)ctab,
                           (const float*)cn2, nc, nctiles, rows.n, ix->dpad, tpb, rows.mask, (const long long*)hdr,
                           ix->km_assign.p, ix->km_dist.p, counts, reinterpret_cast<unsigned long long*>(hdr));
        CSS_LAUNCH_CHECK();
    }
    {
        ProfScope ps("kmeans_lists", st);
        hipLaunchKernelGGL(k_kmeans_offsets, dim3(1), dim3(1024), 0, st, (const unsigned long long*)counts, nc, off, seg);
        CSS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_kmeans_members, dim3((unsigned)((rows.n + 255) / 256)), dim3(256), 0, st,
                           (const int32_t*)ix->km_assign.p, rows.n, (const uint32_t*)off, cursor, ix->km_members.p);
        CSS_LAUNCH_CHECK();
    }
    {
        ProfScope ps("kmeans_sum", st);
        const unsigned grid = (unsigned)(nc + (rows.n + KM_SEG - 1) / KM_SEG);
        hipLaunchKernelGGL(k_kmeans_sum, dim3(grid), dim3(256), 0, st, (const float4*)rows.xb, (const uint32_t*)ix->km_members.p,
                           (const uint32_t*)off, (const uint32_t*)seg, nc, ix->dim, ix->dpad / 4, (const long long*)hdr, sums);
        CSS_LAUNCH_CHECK();
    }
    return CSS_OK;
}
}  // namespace

int css_index_kmeans_step(css_index* ix, const float* centroids_host, int nc, int fx_shift, const uint32_t* allow_bits_host,
                          int64_t* sums_host, int64_t* counts_host, int64_t* obj_host, int* fx_shift_used, int* obj_shift_used,
                          int32_t* assign_host, float* dist_host) {
    CSS_REQUIRE(ix, "css_index_kmeans_step: NULL index");
    CSS_REQUIRE(nc >= 2 && nc <= CSS_MAX_CENTROIDS, "css_index_kmeans_step: nc=%d outside [2, %d]", nc, CSS_MAX_CENTROIDS);
    CSS_REQUIRE(centroids_host && sums_host && counts_host && obj_host, "css_index_kmeans_step: NULL buffer");
    CSS_REQUIRE(fx_shift < 1024, "css_index_kmeans_step: fx_shift=%d out of range", fx_shift);
    for (size_t i = 0, m = (size_t)nc * ix->dim; i < m; ++i)
        CSS_REQUIRE(std::isfinite(centroids_host[i]), "css_index_kmeans_step: centroid %lld has a %s component (column %lld)",
                    (long long)(i / ix->dim), std::isnan(centroids_host[i]) ? "NaN" : "infinite", (long long)(i % ix->dim));
    HostCall hc(ix);
    const hipStream_t st = ix->stream;
    const int64_t n = hc.rows.n;
    long long h[KM_HDR] = {0};
    int rc = hc.upload(allow_bits_host, ix->km_craw, centroids_host, (size_t)nc * ix->dim);
    if (rc == CSS_OK) rc = kmeans_step_enqueue(ix, hc.rows, ix->km_craw.p, nc, fx_shift, st);
    if (rc == CSS_OK) rc = [&]() -> int {   // one wait: header, counts, sums and the per-row arrays the caller asked for
        const long long* out = ix->km_out.p;
        CSS_HIP_TRY(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipMemcpyAsync(counts_host, out + KM_HDR, (size_t)nc * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipMemcpyAsync(sums_host, out + KM_HDR + nc, (size_t)nc * ix->dim * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (assign_host && n) CSS_HIP_TRY(hipMemcpyAsync(assign_host, ix->km_assign.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (dist_host && n) CSS_HIP_TRY(hipMemcpyAsync(dist_host, ix->km_dist.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipStreamSynchronize(st));
        return CSS_OK;
    }();
    if (rc != CSS_OK) return hc.wait_if_failed(rc);
    // an imposed shift that this index's own row count and maximum cannot hold: the sums may have wrapped
    CSS_REQUIRE(h[3] != 0, "css_index_kmeans_step: fx_shift=%d is too large for %lld rows with this index's largest norm: "
                "the largest safe value is %lld", fx_shift, (long long)n, h[4]);
    *obj_host = (int64_t)h[0];
    if (fx_shift_used) *fx_shift_used = (int)h[1];
    if (obj_shift_used) *obj_shift_used = (int)h[2];
    return CSS_OK;
}

namespace {
// The Gram matrix and column sums of the call's rows into gr_out.  Everything is enqueued on `st`; nothing waits for
// the device.  Caller holds ws_mu and a shared lock on mu.
int gram_enqueue(css_index* ix, const Rows& rows, int fx_shift, int gp, hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    // rows appended on another stream must have landed (the running maximum with them)
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    const size_t words = (size_t)GR_HDR + gp + (size_t)gp * gp;
    if ((rc = ix->gr_out.grow(words)) != CSS_OK) return rc;
    long long* hdr = ix->gr_out.p;
    unsigned long long* colsum = reinterpret_cast<unsigned long long*>(hdr + GR_HDR);
    unsigned long long* G = colsum + gp;
    CSS_HIP_TRY(hipMemsetAsync(hdr, 0, words * sizeof(long long), st));
    hipLaunchKernelGGL(k_gram_params, dim3(1), dim3(64), 0, st, (const int*)ix->maxn2.p, rows.n, fx_shift, hdr);
    CSS_LAUNCH_CHECK();
    if (rows.n == 0) return CSS_OK;   // zeros
    const int T = gp / GR_T, ntile = T * (T + 1) / 2;
    // strips: about four blocks per CU over the tiles, at least 512 rows each (a block ends in 16384 atomics), a
    // multiple of the staged chunk; the integers do not depend on this choice
    const int64_t want = std::max<int64_t>(1, (4 * (int64_t)ix->num_cus + ntile - 1) / ntile);
    int64_t rpb = std::max<int64_t>(512, (rows.n + want - 1) / want);
    if (ix->gram_rows > 0) rpb = ix->gram_rows;   // css_index_set_gram_rows: another grid, the same integers
    rpb = (rpb + GR_KC - 1) / GR_KC * GR_KC;
    const int64_t strips = (rows.n + rpb - 1) / rpb;
    CSS_REQUIRE(strips <= 65535, "css_index_gram: internal: %lld strips", (long long)strips);
    ProfScope ps("gram_fx", st);
    hipLaunchKernelGGL(k_gram_fx, dim3((unsigned)ntile, (unsigned)strips), dim3(256), 0, st, rows.xb, rows.n, ix->dpad, gp, rpb,
                       rows.mask, (const long long*)hdr, G, colsum);
    CSS_LAUNCH_CHECK();
    return CSS_OK;
}

// y = A x + b for rows [row0, row0 + n) into y_out_host, in batches of rows through tr_y.  a_dev: the uploaded
// [A | b].  Everything is enqueued on `st`; nothing waits for the device.  Caller holds ws_mu and a shared lock on mu.
int transform_enqueue(css_index* ix, const Rows& rows, const float* a_dev, int m, int64_t row0, int64_t n, float* y_out_host,
                      hipStream_t st) {
    int rc;
    WsTurn turn(ix, st);
    if (turn.rc != CSS_OK) return turn.rc;
    if (ix->ingest_pending) CSS_HIP_TRY(hipStreamWaitEvent(st, ix->ingest_ev, 0));
    CSS_REQUIRE(ix->dpad % MF_BK == 0, "css_index_transform: internal: dpad=%d is no multiple of %d", ix->dpad, MF_BK);
    const int mtiles = (m + MF_BM - 1) / MF_BM, mpad = mtiles * MF_BM;
    if ((rc = ix->tr_tab.grow((size_t)mpad * ix->dpad + 2 * (size_t)mpad)) != CSS_OK) return rc;
    float* atab = ix->tr_tab.p;
    float* an2 = atab + (size_t)mpad * ix->dpad;
    float* bias = an2 + mpad;
    // the table: the row kernel of ingest pads the rows of A (its squared norms go unused); pad rows and pad bias are zero
    CSS_HIP_TRY(hipMemsetAsync(atab + (size_t)m * ix->dpad, 0, ((size_t)(mpad - m) * ix->dpad + 2 * (size_t)mpad) * sizeof(float), st));
    hipLaunchKernelGGL(k_ingest_rows<false>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, a_dev, atab, an2, (int64_t)m,
                       ix->dim, ix->dpad, 0, 0ull, 0ll, (unsigned short*)nullptr, (int*)nullptr, (float*)nullptr,
                       (unsigned char*)nullptr, (float*)nullptr);
    CSS_LAUNCH_CHECK();
    CSS_HIP_TRY(hipMemcpyAsync(bias, a_dev + (size_t)m * ix->dim, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, st));
    const int64_t batch = std::min<int64_t>(n, std::max<int64_t>(MF_BN, ((int64_t)1 << 24) / m / MF_BN * MF_BN));
    if ((rc = ix->tr_y.grow((size_t)batch * m)) != CSS_OK) return rc;
    const size_t lds = (size_t)(2 * MF_BM * MF_BK + 2 * MF_BN * MF_BK + mpad) * 4;
    if ((rc = css::ensure_dynamic_lds((const void*)k_transform_rows, lds, ix->device)) != CSS_OK) return rc;
    for (int64_t r = 0; r < n; r += batch) {
        const int64_t nb = std::min(batch, n - r);
        const int64_t ntiles = (nb + MF_BN - 1) / MF_BN;
        const int64_t want = std::min<int64_t>(ntiles, 2 * (int64_t)ix->num_cus);   // two blocks per CU
        const int64_t tpb = (ntiles + want - 1) / want;
        const unsigned grid = (unsigned)((ntiles + tpb - 1) / tpb);
        {
            ProfScope ps("transform_rows", st);
            hipLaunchKernelGGL(k_transform_rows, dim3(grid), dim3(256), lds, st, rows.xb + (size_t)(row0 + r) * ix->dpad,
                               (const float*)atab, (const float*)bias, m, mtiles, nb, ix->dpad, tpb, ix->tr_y.p);
            CSS_LAUNCH_CHECK();
        }
        CSS_HIP_TRY(hipMemcpyAsync(y_out_host + (size_t)r * m, ix->tr_y.p, (size_t)nb * m * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    return CSS_OK;
}
}  // namespace

int css_index_gram(css_index* ix, int fx_shift, const uint32_t* allow_bits_host, int64_t* gram_host, int64_t* colsum_host,
                   int64_t* count_host, int* fx_shift_used) {
    CSS_REQUIRE(ix, "css_index_gram: NULL index");
    CSS_REQUIRE(gram_host && colsum_host && count_host, "css_index_gram: NULL buffer");
    CSS_REQUIRE(fx_shift < 1024, "css_index_gram: fx_shift=%d out of range", fx_shift);
    HostCall hc(ix);
    const hipStream_t st = ix->stream;
    const int64_t n = hc.rows.n;
    const int dim = ix->dim, gp = (ix->dpad + GR_T - 1) / GR_T * GR_T;
    const size_t words = (size_t)GR_HDR + gp + (size_t)gp * gp;
    const std::unique_ptr<long long[]> h(new (std::nothrow) long long[words]);
    if (!h) {
        css::set_error("css_index_gram: no host memory for %zu bytes of results", words * sizeof(long long));
        return CSS_ERR_OOM;
    }
    hc.enqueued = true;
    int rc = upload_allow_bits(ix, allow_bits_host, &hc.rows);
    if (rc == CSS_OK) rc = gram_enqueue(ix, hc.rows, fx_shift, gp, st);
    if (rc == CSS_OK) rc = [&]() -> int {   // one wait
        CSS_HIP_TRY(hipMemcpyAsync(h.get(), ix->gr_out.p, words * sizeof(long long), hipMemcpyDeviceToHost, st));
        CSS_HIP_TRY(hipStreamSynchronize(st));
        return CSS_OK;
    }();
    if (rc != CSS_OK) return hc.wait_if_failed(rc);
    // an imposed shift that this index's own row count and maximum cannot hold: the sums may have wrapped
    CSS_REQUIRE(h[1] != 0, "css_index_gram: fx_shift=%d is too large for %lld rows with this index's largest norm: "
                "the largest safe value is %lld", fx_shift, (long long)n, h[2]);
    // the device fills the upper TILE triangle; the rest is its mirror image.  Pad columns stay behind.
    const long long* cs = h.get() + GR_HDR;
    const long long* G = cs + gp;
    for (int i = 0; i < dim; ++i) {
        colsum_host[i] = (int64_t)cs[i];
        for (int j = 0; j < dim; ++j)
            gram_host[(size_t)i * dim + j] = (int64_t)(i / GR_T <= j / GR_T ? G[(size_t)i * gp + j] : G[(size_t)j * gp + i]);
    }
    int64_t count = n;
    if (allow_bits_host && n > 0) {
        count = 0;
        for (int64_t w = 0, words = (n + 31) / 32; w < words; ++w) {
            uint32_t bits = allow_bits_host[w];
            if (w == words - 1 && (n & 31)) bits &= (1u << (n & 31)) - 1u;
            count += __builtin_popcount(bits);
        }
    }
    *count_host = count;
    if (fx_shift_used) *fx_shift_used = (int)h[0];
    return CSS_OK;
}

int css_index_transform(css_index* ix, const float* A_host, const float* b_host, int m, int64_t row0, int64_t n,
                        float* y_out_host) {
    CSS_REQUIRE(ix, "css_index_transform: NULL index");
    CSS_REQUIRE(m >= 1 && m <= CSS_MAX_TRANSFORM_ROWS, "css_index_transform: m=%d outside [1, %d]", m, CSS_MAX_TRANSFORM_ROWS);
    CSS_REQUIRE(A_host, "css_index_transform: NULL matrix");
    for (size_t i = 0, e = (size_t)m * ix->dim; i < e; ++i)
        CSS_REQUIRE(std::isfinite(A_host[i]), "css_index_transform: row %lld of A has a %s component (column %lld)",
                    (long long)(i / ix->dim), std::isnan(A_host[i]) ? "NaN" : "infinite", (long long)(i % ix->dim));
    for (int c = 0; b_host && c < m; ++c)
        CSS_REQUIRE(std::isfinite(b_host[c]), "css_index_transform: entry %d of b is %s", c, std::isnan(b_host[c]) ? "NaN" : "infinite");
    HostCall hc(ix);
    CSS_REQUIRE(row0 >= 0 && n >= 0 && row0 + n <= hc.rows.n, "css_index_transform: rows [%lld, %lld) outside [0, %lld)",
                (long long)row0, (long long)(row0 + n), (long long)hc.rows.n);
    if (n == 0) return CSS_OK;
    CSS_REQUIRE(y_out_host, "css_index_transform: NULL buffer");
    const size_t nab = (size_t)m * ix->dim + m;   // [A | b], b = 0 without one: one upload
    const std::unique_ptr<float[]> ab(new (std::nothrow) float[nab]);
    if (!ab) {
        css::set_error("css_index_transform: no host memory for %zu bytes of [A | b]", nab * sizeof(float));
        return CSS_ERR_OOM;
    }
    memcpy(ab.get(), A_host, (size_t)m * ix->dim * sizeof(float));
    if (b_host) memcpy(ab.get() + (size_t)m * ix->dim, b_host, (size_t)m * sizeof(float));
    else memset(ab.get() + (size_t)m * ix->dim, 0, (size_t)m * sizeof(float));
    int rc = hc.upload(nullptr, ix->tr_raw, (const float*)ab.get(), nab);
    if (rc == CSS_OK) rc = transform_enqueue(ix, hc.rows, ix->tr_raw.p, m, row0, n, y_out_host, ix->stream);
    if (rc == CSS_OK) rc = [&]() -> int {
        CSS_HIP_TRY(hipStreamSynchronize(ix->stream));
        return CSS_OK;
    }();
    return hc.wait_if_failed(rc);
}

}  // extern "C"
