/*
 * css_hip.h -- C ABI of libcss_hip.so, the MI355X (gfx950) implementation of the
 * embed-and-search hot path of pauloportella/claude-semantic-search.
 *
 * The reference is pure Python; its arithmetic is reached through two third
 * party seams.  Each entry point below names the reference
 * call site it replaces (paths relative to the reference checkout):
 *
 *   faiss.IndexFlatIP(d) / IndexFlatL2(d)    src/storage.py:252-258  -> css_index_create
 *   faiss_index.add(x)                       src/storage.py:359      -> css_index_add
 *   x / (norm + 1e-8) row-normalise          src/storage.py:347-350  -> css_index_add(normalize=1)
 *   faiss_index.ntotal                       src/storage.py:358,421  -> css_index_ntotal
 *   q / (norm + 1e-8), reshape(1,-1)         src/storage.py:424-429  -> css_index_search(normalize_q=1)
 *   faiss_index.search(q, k) -> (D, I)       src/storage.py:436      -> css_index_search
 *   faiss_index.range_search(q, r)           (not called by the reference) -> css_index_range_search
 *   (no faiss call: facet counts per query)  (not called by the reference) -> css_index_facets
 *   _matches_filters(chunk, filters) per row src/storage.py:508-543  -> css_index_set_attr + css_index_where
 *   faiss.write_index / read_index payload   src/storage.py:306,879  -> css_index_export / css_index_add
 *   faiss.index_cpu_to_gpu / get_num_gpus    src/storage.py:283, src/gpu_utils.py:117-118
 *                                                                    -> css_device_count / css_device_info
 *   SentenceTransformer(name).encode(...)    src/embeddings.py:184-188, :216-222
 *                                                                    -> css_encoder_forward
 *   model.get_sentence_embedding_dimension() src/embeddings.py:117   -> css_encoder_cfg.hidden
 *
 * Conventions: extern "C", opaque handles, plain pointers and sizes.  Every
 * function returns 0 on success or a negative css_status; the message for the
 * calling thread is available from css_last_error().  Host pointers are caller
 * owned and are consumed before return.  "_dev" twins take device pointers and
 * a hipStream_t (as void*) and enqueue asynchronously on that stream; they are
 * what a PyTorch-ROCm host passes tensor.data_ptr() / current_stream to.
 * There is NO CPU fallback in this library: with no HIP device every compute
 * entry point fails with CSS_ERR_NO_DEVICE.
 */
#ifndef CSS_HIP_H
#define CSS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum css_status {
    CSS_OK = 0,
    CSS_ERR_INVALID = -1,   /* bad argument */
    CSS_ERR_NO_DEVICE = -2, /* no usable HIP device */
    CSS_ERR_HIP = -3,       /* HIP runtime error (message has the hipError string) */
    CSS_ERR_OOM = -4,       /* device allocation failed */
    CSS_ERR_STATE = -5      /* object not in a state that allows the call */
} css_status;

enum { CSS_METRIC_IP = 0, CSS_METRIC_L2 = 1 };

/* Largest k accepted by css_index_search.  The reference asks for
 * k' = min(SearchConfig.max_results, ntotal) (src/storage.py:432; max_results
 * defaults to 100, :69, and may be set to anything).  Up to 128 a search is one
 * pass of the scan kernels; beyond, every query takes ceil(k / 128) passes over
 * the rows the earlier passes did not return (still exact, still enqueue-only). */
#define CSS_MAX_K 2048

typedef struct css_devinfo {
    char name[128];
    char gcn_arch[64];
    int compute_units;
    int wavefront_size;
    int64_t hbm_total_bytes;
    int64_t hbm_free_bytes;
    int lds_bytes_per_cu;
    int clock_mhz;
} css_devinfo;

typedef struct css_index css_index;
typedef struct css_encoder css_encoder;

const char* css_version(void);
const char* css_last_error(void);

int css_device_count(int* n);
int css_device_info(int device, css_devinfo* out);

/* ---- flat exact index (IndexFlatIP / IndexFlatL2 semantics) ---- */
int css_index_create(int dim, int metric, int device, css_index** out);
int css_index_free(css_index* ix);
int css_index_reset(css_index* ix);                 /* ntotal := 0, keeps capacity */
int css_index_reserve(css_index* ix, int64_t n);    /* capacity >= n rows, no copy later */
/* faiss IndexFlat::remove_ids: drop the rows whose bit is CLEAR in keep_bits (layout of allow_bits: bit (r & 31)
 * of word r >> 5, local row numbering, ceil(ntotal / 32) words, host memory; bits beyond ntotal are ignored);
 * surviving rows keep their order and move down, so row r becomes row r - (removed rows below r).
 * *removed_out = number of rows dropped.  In place on the device: capacity and id_base are kept, rows below the
 * first removed one are not moved, and the index ends in the state of one freshly built from the survivors (the
 * reduced-precision row copies and the error-band maxima included).  Extra device memory does not grow with
 * ntotal: at most 128 MiB of bounce rows (the staging buffer of css_index_add) and 4 MiB of keep bits and their
 * prefix counts.  Waits for pending adds and searches and for its own work before it returns. */
int css_index_remove_rows(css_index* ix, const uint32_t* keep_bits_host, int64_t* removed_out);
/* Diagnostics: the three running maxima the error bands are built from (max ||x||^2, max ||x - bf16(x)||^2,
 * max ||x - int8(x)||^2) as floats.  Waits for the device. */
int css_index_bounds(css_index* ix, float out[3]);
int css_index_ntotal(const css_index* ix, int64_t* n);
int css_index_dim(const css_index* ix, int* dim);
int css_index_metric(const css_index* ix, int* metric);
int css_index_device(const css_index* ix, int* device);
/* Diagnostics: how many queries of the LAST candidate-path search (its last chunk of up to 4096 queries) overflowed
 * their candidate buffer or band (and were settled by the second coarse pass or the exact sweep).  Waits for the device. */
int css_index_last_flagged(css_index* ix, int64_t* n);
/* ... and how many of those the second coarse pass could not settle either (candidate buffers of 32768 rows
 * overflowed, or more than 1024 flagged queries in a chunk): these were re-run by the exact fp32 sweep. */
int css_index_last_swept(css_index* ix, int64_t* n);
/* Reduced-precision copies of the rows, the operands of the candidate scans (results never depend on them: candidates
 * come from a scan inside an error band measured at ingest and are rescored in fp32):
 *   bf16 rows (+50 % HBM next to the fp32 rows) and INT8 rows (signed byte = round(x / s), s = max|x| / 127 per row;
 *   +25 %; rows of at most 1024 elements).  Searches of 1..4 queries sweep the int8 rows (one query: the whole stage
 *   cascade in one persistent kernel launch, css_knn_coarse.h: k_sweep_cascade), 3..32 inner-product queries sweep them on
 *   the int8 MFMA with the queries as the register operand (k_sweep_mfma_i8); batches scan them with int8
 *   MFMA (rows of 256 / 512 / 768 elements: the queries resident in registers, k_scan_qreg_i8) where that pays (inner product, rows a multiple of 256 elements: k <= 32 from 300 k rows, k <= 128 from 2 M rows; an index whose int8 searches flag more than 5 % of their queries falls back to the bf16 rows
 *   for the next 16 searches), otherwise the bf16 rows.
 * policy: -1 = automatic -- both copies while 7 bytes per element fit in 80 % of the HBM, bf16 only at 6 bytes, INT8 ONLY
 * at 5 bytes (inner product, rows a multiple of 256 elements: ~38-46 M rows of 768 floats on a 288 GB GPU), nothing
 * beyond (batches then round row ranges into scratch memory per search); 0 = never any copy; 1 = always bf16 (+ int8
 * while it fits); 2 = int8 rows only.  Only on an empty index. */
int css_index_set_shadow(css_index* ix, int policy);
/* Diagnostics: which reduced-precision copies of the rows the index currently holds (0 / 1 each). */
int css_index_shadow_info(css_index* ix, int* has_bf16, int* has_int8);
/* Global id of local row 0 (shards of a row-partitioned index). */
int css_index_set_id_base(css_index* ix, int64_t base);

/* Append n rows (row-major [n, dim] fp32).  normalize != 0 applies the
 * reference's x / (||x||_2 + 1e-8) per row on the device while copying in. */
int css_index_add(css_index* ix, const float* x_host, int64_t n, int normalize);
int css_index_add_dev(css_index* ix, const float* x_dev, int64_t n, int normalize, void* stream);
/* Append n rows generated on the device from include/css_synth.h:
 * row r, column c = css_synth_normal(seed, (first_row + r) * dim + c). */
int css_index_add_synthetic(css_index* ix, int64_t n, uint64_t seed, int64_t first_row,
                            int normalize, void* stream);
/* Copy rows [row0, row0 + n) back to the host as [n, dim] fp32. */
int css_index_export(const css_index* ix, int64_t row0, int64_t n, float* x_out_host);

/* Exact top-k.  IP: D descending inner products.  L2: D ascending squared
 * distances.  Ties: lower id first.  Fewer than k rows: I = -1 and
 * D = -FLT_MAX (IP) / +FLT_MAX (L2).  1 <= k <= CSS_MAX_K.
 * normalize_q != 0 applies q / (||q||_2 + 1e-8) first (src/storage.py:426).
 * Indexes keep a bf16 shadow copy of the rows while it fits in HBM; searches
 * of large indexes then select candidates with a bf16 scan inside a rigorous
 * error band and return exact fp32 scores of the rescored candidates (same
 * results as the fp32 kernels).  Without shadow rows, batches round the rows to
 * bf16 one row range at a time into scratch memory and run the same scan per range.  The _dev form only enqueues on `stream` and never
 * waits for the device (one exception: the FIRST batched search of an index without shadow rows allocates that scratch
 * -- up to half of the free HBM -- and a growing workspace is reallocated; hipMalloc / hipFree synchronise the device.
 * Later searches of the same shapes allocate nothing): queries whose candidate band overflows are re-run exactly by
 * one launch that follows every cascade and returns at once when there are none.
 * Rows appended by css_index_add_dev / css_index_add_synthetic on another stream are
 * ordered before the search by an event (no caller-side synchronisation needed); successive
 * asynchronous adds on different streams are chained the same way.
 * All searches of one index share one set of device workspaces: a search enqueued on a
 * different stream than the previous one first waits (on the device, by an event) for that
 * search to finish, so searches of ONE index execute one after the other whatever streams
 * they are given -- use one index per concurrent stream (or shard) for overlap.  D_dev /
 * I_dev belong to the caller: read them after synchronising with `stream` as usual. */
/* Search path: CSS_SEARCH_AUTO (default) selects candidates with a reduced-precision scan
 * inside a rigorous error band and rescores them in fp32 where the multi-launch cascade
 * pays (5 or more queries, or k > 32: always; 1..4 queries with k <= 32: from 100 k rows;
 * rows are kept as fp32 + bf16 + int8 copies where the HBM allows); CSS_SEARCH_EXACT_FP32 forms every score
 * with fp32 fmaf chains inside the scan kernels (VALU sweeps up to 16 queries, fp32-input
 * MFMA beyond; the parity mode of the tests, and what small indexes use for few queries). */
#define CSS_SEARCH_AUTO 0
#define CSS_SEARCH_EXACT_FP32 1
#define CSS_SEARCH_COARSE 2 /* the candidate path whatever the index size (AUTO uses it only where it pays) */
#define CSS_SEARCH_SPLIT 3  /* batches of > 16 queries: candidates from split-operand (bf16 pair) products of the fp32 rows +
                               fp32 rescoring -- what an index without shadow rows falls back to when no HBM is left for
                               the scratch rows of its bf16 ranges; selectable for verification */
int css_index_set_search_mode(css_index* ix, int mode);
/* Indexes without shadow rows: rows per bf16 scratch range of a batched search (0 = automatic: half of the free HBM,
 * at most 2^24 rows).  A tuning / verification knob: results do not depend on it. */
int css_index_set_range_rows(css_index* ix, int64_t rows);
int css_index_search(css_index* ix, const float* q_host, int64_t nq, int k, int normalize_q,
                     float* D_host, int64_t* I_host);
int css_index_search_dev(css_index* ix, const float* q_dev, int64_t nq, int k, int normalize_q,
                         float* D_dev, int64_t* I_dev, void* stream);

/* Masked search (filter / tombstone push-down; the reference
 * instead over-fetches 100 hits and filters them afterwards, src/storage.py:438-492):
 * only rows whose bit is set in allow_bits -- bit (r & 31) of word r >> 5, local row
 * numbering, ceil(ntotal / 32) words -- can be returned; NULL = all rows.  Fewer than
 * k allowed rows: padded like css_index_search. */
int css_index_search_masked(css_index* ix, const float* q_host, int64_t nq, int k, int normalize_q,
                            const uint32_t* allow_bits_host, float* D_host, int64_t* I_host);
int css_index_search_masked_dev(css_index* ix, const float* q_dev, int64_t nq, int k, int normalize_q,
                                const uint32_t* allow_bits_dev, float* D_dev, int64_t* I_dev,
                                void* stream);

/* Search by id ("related rows"; what faiss users write as search-by-id-excluding-self): query j is the stored fp32 row
 * whose GLOBAL id is ids[j] (id_base included), exactly as it lies in HBM.
 *  - No query normalisation is applied; repeated ids are allowed.  The result has the layout and order of
 *    css_index_search_masked (D[nq,k], I[nq,k], IP descending / L2 ascending squared distance, ties to the lower id,
 *    -1 with -FLT_MAX / +FLT_MAX padding), and allow_bits (may be NULL) means what it means there.
 *  - exclude_self != 0: id ids[j] never appears in row j, and the row is the exact top-k of (allowed rows minus the
 *    anchor).  Exact duplicates of the anchor stored under other ids are ordinary results; the anchor itself need not be
 *    allowed by allow_bits.  The search runs for k + 1, so 1 <= k <= CSS_MAX_K - 1 (k == CSS_MAX_K: CSS_ERR_INVALID).
 *  - exclude_self == 0: the result of css_index_search_masked with those rows as queries; 1 <= k <= CSS_MAX_K.
 *  - Three steps on the device: one wave per anchor gathers its row into a query buffer, the search of
 *    css_index_search_masked_dev runs unchanged on that buffer (search mode, reduced-precision copies, k > 128 passes
 *    and query chunking as there), one wave per query then drops the anchor -- or, where the anchor is not among the
 *    k + 1 (masked out, or an inner-product row that is not its own best match), the last entry.
 *  - Host form: an id outside [id_base, id_base + ntotal) is CSS_ERR_INVALID, the message names the id, and nothing is
 *    enqueued (so every call on an empty index with nq > 0 fails).  Device form: the ids cannot be looked at without
 *    a wait, so a query with an invalid id returns a fully padded row, its neighbours are unaffected (an empty index:
 *    every row padded), and the call waits for the device no more than css_index_search_masked_dev does.
 *  - nq == 0 is a no-op.  Rows appended on other streams, the serialisation of the searches of one index and the
 *    shared workspaces are those of css_index_search_masked_dev. */
int css_index_search_rows(css_index* ix, const int64_t* ids_host, int64_t nq, int k, int exclude_self,
                          const uint32_t* allow_bits_host, float* D_host, int64_t* I_host);
int css_index_search_rows_dev(css_index* ix, const int64_t* ids_dev, int64_t nq, int k, int exclude_self,
                              const uint32_t* allow_bits_dev, float* D_dev, int64_t* I_dev, void* stream);

/* Group labels and grouped search ("which conversations are nearest": Elasticsearch "collapse", Qdrant "search groups",
 * Milvus "grouping search"): the best row of each of the k best groups, exactly.
 *  - Labels.  Every row has an int32 group label.  A row that was never given one has -1, and so does a row given a
 *    negative one; each such row is a group of its own and never collapses with anything.  Labels are per index, in
 *    LOCAL row numbering like allow_bits (id_base plays no part).  css_index_set_groups writes the labels of rows
 *    [row0, row0 + n), css_index_get_groups reads them back; a range outside [0, ntotal) is CSS_ERR_INVALID.  Both wait
 *    for pending asynchronous adds; set takes the index exclusively (like css_index_add), get shares it (like
 *    css_index_export).  The column (4 bytes per row of capacity) is allocated by the first css_index_set_groups: an
 *    index that never sets labels pays nothing.  It follows the rows: kept through capacity growth, -1 for appended
 *    rows, compacted by css_index_remove_rows with the same keep bits (afterwards get_groups = labels[keep]),
 *    forgotten by css_index_reset.
 *  - css_index_search_grouped.  For every query: the k best groups among the allowed rows.  A group is ranked by its
 *    best allowed row under the index's total order (score, then lower id); the output is that row's score D, its
 *    GLOBAL id I and the group's label G (-1 for an ungrouped row; G_host may be NULL).  Layout, order, tie rule and
 *    padding are those of css_index_search_masked (I = -1, D = -FLT_MAX / +FLT_MAX) with G = -1 in padded slots;
 *    normalize_q and allow_bits_host mean what they mean there.  1 <= k <= 128 (the kernels' list size), anything else
 *    is CSS_ERR_INVALID.  Fewer than k groups among the allowed rows: a padded tail.  An empty index: fully padded
 *    rows.  nq == 0 is a no-op.  An index with no labels at all returns exactly what css_index_search_masked returns
 *    for the same k.
 *  - Exactness.  In a best-first list of the top kk rows the first occurrences of distinct groups are exactly the best
 *    groups, each with its best row, and every group that is absent has its best row below entry kk -- so the result
 *    is exact whatever over-fetch is used.  Pass 1 searches the whole batch for kk rows (32 when 2k <= 32, else 128)
 *    and collapses them on the device.  A query that then has neither k groups nor a padded list goes on alone: every
 *    further pass searches 128 rows under an exclusion bitmap from which ALL rows of the groups already found were
 *    dropped, so it brings at least one new group (at most k passes per query; one group that fills the lists costs
 *    one extra pass, not one pass per 128 of its rows).  Queries that took several passes are sorted once more.
 *  - The pass count depends on the data, so only a host form exists: it waits for the device between passes.
 *    css_index_last_group_passes: search passes of the last grouped call (1 when pass 1 sufficed for every query). */
int css_index_set_groups(css_index* ix, int64_t row0, int64_t n, const int32_t* labels_host);
int css_index_get_groups(css_index* ix, int64_t row0, int64_t n, int32_t* labels_out_host);
int css_index_search_grouped(css_index* ix, const float* q_host, int64_t nq, int k, int normalize_q,
                             const uint32_t* allow_bits_host, float* D_host, int64_t* I_host,
                             int32_t* G_host /* may be NULL */);
int css_index_last_group_passes(css_index* ix, int64_t* n);   /* diagnostics: search passes of the last grouped call */

/* Per-row priors and prior-weighted search (Elasticsearch "function score", Vespa rank-profile freshness terms, a
 * document prior): the k best rows under the query score PLUS a per-row additive term -- "prefer the recent ones" is
 * one use of it.  A re-rank of an over-fetched list cannot do this: a boosted row may sit anywhere below the fetched
 * rows, so the fused value is the key of the sweep itself.
 *  - Priors.  Every row has one fp32 prior; a row never given one has 0.0f.  Priors are per index, in LOCAL row
 *    numbering like allow_bits and the group labels.  css_index_set_priors writes the priors of rows [row0, row0 + n),
 *    css_index_get_priors reads them back; a range outside [0, ntotal) is CSS_ERR_INVALID.  A NaN or infinite value is
 *    CSS_ERR_INVALID: the message names the row and NOTHING is written.  Locking and the ordering against pending
 *    asynchronous adds are those of css_index_set_groups / css_index_get_groups.  The column (4 bytes per row of
 *    capacity) is allocated by the first css_index_set_priors: an index that never sets one pays nothing, and its
 *    get_priors returns zeros without touching the device.  It follows the rows: kept through capacity growth, 0.0f for
 *    appended rows, compacted by css_index_remove_rows with the same keep bits (afterwards get_priors = priors[keep],
 *    bit for bit), forgotten by css_index_reset.
 *  - css_index_search_prior.  For every query the k best allowed rows under the FUSED value, with p_r the row's prior:
 *        inner product   f = fmaf(weight, p_r, s)       larger is better
 *        squared L2      f = fmaf(-weight, p_r, dist)   smaller is better: a positive prior pulls a row closer, and f
 *                                                       may be negative
 *    s / dist is the exact fp32 score of the fp32 rows, in the arithmetic of CSS_SEARCH_EXACT_FP32 for up to 16 queries
 *    (one fmaf chain per lane over the padded row, the row reduction, L2 from differences).  D = f, best first, ties to
 *    the lower id; I = global ids; S (may be NULL) = the row's raw s / dist, so that thresholds keep their meaning:
 *    D[j, t] is exactly the fmaf above applied to S[j, t].  Padding as in css_index_search: I = -1 and D = S = -FLT_MAX
 *    (inner product) / +FLT_MAX (L2).
 *  - Limits: 1 <= k <= 128 (the kernels' list size); weight is any finite float (NaN or infinity is CSS_ERR_INVALID,
 *    the message names it).  nq == 0 is a no-op; an empty index gives fully padded rows.  normalize_q, allow_bits_host,
 *    rows appended on other streams and the shared workspaces are those of css_index_search_masked.
 *  - Nothing depends on the reduced-precision row copies (css_index_set_shadow) or on the search mode.  An index without
 *    priors, or weight == 0, gives f == s bit for bit: the result of css_index_search under CSS_SEARCH_EXACT_FP32 for up
 *    to 16 queries, with S == D.
 *  - On the device: one sweep of the fp32 rows serves up to 16 queries (longer batches are walked a sweep at a time: a
 *    correctness path, the workload is one query); it reads 4 * dpad + 4 bytes per row.  The raw scores of the nq * k
 *    returned rows are re-formed by one small launch behind the merge, with the sweep's own summation order.  There is
 *    no candidate path: a certified over-fetch would need a bound on weight * max prior below the score spread of the
 *    best rows. */
int css_index_set_priors(css_index* ix, int64_t row0, int64_t n, const float* priors_host);
int css_index_get_priors(css_index* ix, int64_t row0, int64_t n, float* priors_out_host);
int css_index_search_prior(css_index* ix, const float* q_host, int64_t nq, int k, float weight, int normalize_q,
                           const uint32_t* allow_bits_host, float* D_host, int64_t* I_host,
                           float* S_host /* may be NULL */);

/* Search by examples (the "recommend" / "more like these" / positive-negative-examples call of vector stores): the k
 * best rows for a SET of example vectors, some of them to be avoided -- "more like these three chunks, and not like
 * that one", "anything that matches any of these phrasings".  One request per call.
 *  - Examples.  m = npos + nneg of them, 1 <= npos, m <= CSS_MAX_EXAMPLES.  Each is a caller's vector ([d] fp32;
 *    normalize_vec != 0: x / (||x|| + 1e-8) as in css_index_search) or a stored row named by its GLOBAL id, taken as it
 *    lies in device memory, never normalised, gathered on the device.  vec_host holds the nvec_pos positive vectors and
 *    then the nvec_neg negative ones, ids_host the nid_pos positive ids and then the nid_neg negative ones (either may
 *    be NULL when it holds nothing).  Order of the examples: positive vectors, positive ids, negative vectors, negative
 *    ids.
 *  - The value.  With s_j the score of a row against example j (the exact fp32 score of the fp32 rows, in the
 *    arithmetic of CSS_SEARCH_EXACT_FP32: the inner product, or the squared L2 distance):
 *        inner product   P = max over positives of s_j, N = max over negatives of s_j     larger f is better
 *        squared L2      P = min over positives of s_j, N = min over negatives of s_j     smaller f is better; f may be < 0
 *        f = P when nneg == 0, else f = fmaf(-gamma, N, P)
 *    The k best ALLOWED rows under f, exact over all rows (the fused value is the key of the sweep: a row's value
 *    under the negatives can sit anywhere below an over-fetched list, and a maximum of scores is not the score of a
 *    combined vector).  D = f, best first, ties to the lower id; I = global ids; S (may be NULL) = P, the raw best
 *    positive score, so that similarity thresholds keep their meaning: D[t] == S[t] bit for bit when nneg == 0, and
 *    D[t] == fmaf(-gamma, N, S[t]) otherwise.  All three are [k].  Padding as in css_index_search: I = -1 and
 *    D = S = -FLT_MAX (inner product) / +FLT_MAX (L2).
 *  - exclude_ids != 0: the rows named as id examples (positive and negative) are never returned.  Copies of them under
 *    other ids are ordinary results; vector examples exclude nothing.  allow_bits_host applies to the answer, not to
 *    the examples: an example id need not be allowed itself.
 *  - CSS_ERR_INVALID, checked on the host before anything is enqueued (the index stays usable): an id outside the index
 *    (the message names it), no positive, m > CSS_MAX_EXAMPLES, k outside [1, 128], a NaN, infinite or negative gamma,
 *    more than 2^32 - 2 rows, and an example table beyond the sweep's 64 KiB of LDS (16 examples: d <= 960; 8: d <= 1984).
 *    An empty index gives fully padded output (and knows no id).
 *  - Nothing depends on the reduced-precision row copies or on the search mode.  One positive vector and no negative is
 *    css_index_search under CSS_SEARCH_EXACT_FP32 bit for bit; gamma == 0 is the call without its negatives.
 *  - On the device: the example table is assembled from one upload (the vectors through the query preparation, the id
 *    examples gathered row to row), ONE sweep of the fp32 rows forms the m scores of every row and keeps one list, and
 *    one small launch behind the merge re-forms P of the k returned rows with the sweep's summation order (skipped when
 *    S_host is NULL).  One wait. */
#define CSS_MAX_EXAMPLES 16
int css_index_search_examples(css_index* ix, const float* vec_host, int nvec_pos, int nvec_neg, const int64_t* ids_host,
                              int nid_pos, int nid_neg, int k, float gamma, int normalize_vec, int exclude_ids,
                              const uint32_t* allow_bits_host, float* D_host, int64_t* I_host,
                              float* S_host /* may be NULL */);

/* Per-row term lists and hybrid search (the BM25 side that Elasticsearch, Vespa, Qdrant and Milvus pair with their
 * dense search): the k best rows under the query score PLUS alpha times a BM25 score of the query's terms against the
 * row's term list -- "which chunks contain hipErrorIllegalAddress" is a question a sentence encoder blurs.  As with the
 * priors, a re-rank of an over-fetched dense list cannot do this: a row that holds a rare query term may sit anywhere
 * below the fetched rows, so the fused value is the key of the sweep itself.
 *  - Term lists.  A term is a uint32 below CSS_TERM_SPACE (2^24); what a term means (a hashed word) is the caller's.
 *    Every row may carry the distinct terms of its text, each with a term frequency, and its length dl = the number of
 *    tokens it was given, repeats included (at most CSS_MAX_ROW_TOKENS).  Stored per row: one uint32 per distinct term,
 *    term << 8 | min(tf, 255), ascending by term, and one uint32 dl.  Lists are per index, in LOCAL row numbering, and
 *    APPEND-ONLY in row order: with T the number of leading rows that have lists, css_index_set_terms takes the raw
 *    tokens of rows [row0, row0 + n) as CSR (offsets_host [n + 1] from 0, tokens_host; repeats, any order and empty rows
 *    are allowed; the library sorts and counts each row on the host).  row0 == T appends; row0 < T first drops the lists
 *    of ALL rows >= row0, then appends (row0 = 0 is the rewrite); row0 > T and a range outside [0, ntotal) are
 *    CSS_ERR_INVALID.  Rows >= T have the empty list and dl = 0.  Offsets that do not start at 0 or that decrease, a
 *    token >= 2^24 (the message names the row) and a row of more than 2^20 tokens are CSS_ERR_INVALID, checked before
 *    anything is written.  Locking and the ordering against pending asynchronous adds are those of css_index_set_groups.
 *    css_index_get_terms reads the stored form of rows [row0, row0 + n) back: offsets_out [n + 1] from 0, the packed
 *    entries and dl (either may be NULL).
 *  - Storage.  Nothing is allocated before the first css_index_set_terms: an index that never receives terms pays
 *    nothing.  Then: 4 bytes per entry, 12 per row with a list, and the statistics, a table df[2^24] of uint32 (64 MB:
 *    the rows that hold a term) and a 64-bit total_len (the sum of dl), kept current by integer atomics, one add per
 *    entry of the lists that come or go (integer sums do not depend on arrival order).  The lists follow the rows:
 *    kept through capacity growth, none for appended rows, forgotten by css_index_reset, compacted by
 *    css_index_remove_rows with the same keep bits -- afterwards css_index_get_terms and css_index_term_stats equal those
 *    of a fresh index built from the kept rows and their lists (T becomes the kept rows below the old T).  The library
 *    mirrors the row offsets on the host (8 bytes per row with a list).
 *  - css_index_term_stats: df of the m asked terms (m <= 2^20), ndocs = ntotal, total_len.  Without lists: zeros, and
 *    no device is touched.  The BM25 weights (an idf per term) are the caller's: lexical.bm25_weights.
 *  - css_index_search_hybrid.  One request per call.  With m <= CSS_MAX_QUERY_TERMS distinct terms t_j and finite
 *    weights w_j, and tf_j the STORED (saturated) count of t_j in row r, all in fp32 and in this order of operations
 *    (the library is built with -ffp-contract=off; fp32 division is correctly rounded):
 *        c0 = k1 * (1.0f - b);   c1 = (k1 * b) / avgdl;
 *        K  = c0 + c1 * (float)dl_r;
 *        g_j = ((float)tf_j * (k1 + 1.0f)) / ((float)tf_j + K);
 *        lex_r = 0.0f;  for j = 0 .. m-1 in the caller's order:  if (tf_j > 0) lex_r = lex_r + w_j * g_j;
 *    The sum runs in QUERY-TERM order, whatever the order of the entries in memory, so a float32 restatement gives the
 *    same bits and a shard gives the same bits as one index.  The k best allowed rows under
 *        inner product   f = fmaf(alpha, lex_r, s)        larger is better
 *        squared L2      f = fmaf(-alpha, lex_r, dist)    smaller is better; f may be negative
 *    which is css_index_search_prior with the lexical column in the place of the priors (the stored priors play no part
 *    in this call).  D = f, best first, ties to the lower id; I = global ids; S (may be NULL) = the raw s / dist;
 *    L (may be NULL) = lex of the returned rows; all [k].  Padding as in css_index_search_prior, with L = 0.
 *  - Limits: 1 <= k <= 128; 0 <= m <= 32; alpha finite; k1 finite and >= 0; 0 <= b <= 1; avgdl finite and > 0; a NaN or
 *    infinite value is CSS_ERR_INVALID and the message names which; a repeated query term is CSS_ERR_INVALID and the
 *    message names it.  An empty index gives fully padded rows.  normalize_q and allow_bits_host are those of
 *    css_index_search_prior.
 *  - m == 0, alpha == 0 or an index without lists give css_index_search_prior on an index without priors bit for bit,
 *    with S == D and L == 0.  Nothing depends on the reduced-precision row copies or on the search mode.
 *  - On the device: k_lex_scores makes one pass over the lists (4 bytes per entry, 12 per row read, 4 per row written)
 *    into a workspace column, the prior sweep runs with that column, one small launch gathers L.  A search never edits
 *    the index.  One wait. */
#define CSS_TERM_SPACE (1u << 24)
#define CSS_MAX_ROW_TOKENS (1 << 20)
#define CSS_MAX_QUERY_TERMS 32
int css_index_set_terms(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host /* [n+1] */,
                        const uint32_t* tokens_host);
int css_index_get_terms(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out /* [n+1], from 0 */,
                        uint32_t* entries_out /* may be NULL */, uint32_t* dl_out /* may be NULL */);
int css_index_term_stats(css_index* ix, const uint32_t* terms_host, int m, int64_t* df_out /* [m] */, int64_t* ndocs_out,
                         int64_t* total_len_out);
int css_index_search_hybrid(css_index* ix, const float* q_host /* [dim] */, int k, float alpha, const uint32_t* terms_host,
                            const float* weights_host, int m, float k1, float b, float avgdl, int normalize_q,
                            const uint32_t* allow_bits_host, float* D_host, int64_t* I_host,
                            float* S_host /* may be NULL */, float* L_host /* may be NULL */);

/* Per-row sparse vectors and sparse search (learned sparse retrieval as a FIRST stage and as the sparse leg of hybrid
 * search: OpenSearch neural sparse, Qdrant and Milvus sparse vectors, Vespa, ELSER).  A row may carry a sparse vector,
 * (term, weight) pairs such as SparseEncoder.encode produces; a query is a sparse vector too, and a row's value is the
 * dot product of the two.  A second per-row list kind, independent of the term lists above: an index may carry both,
 * either or neither.
 *  - Vectors.  A term is a uint32 below CSS_TERM_SPACE; a stored weight is finite, > 0 and <= CSS_MAX_SPARSE_WEIGHT (a
 *    zero weight means "not in the vector" and is refused, not stored); at most CSS_MAX_SPARSE_ROW_ENTRIES entries per
 *    row, terms distinct within a row.  Stored per entry: 8 bytes, (uint32 term, float weight), ascending by term.
 *    css_index_set_sparse takes rows [row0, row0 + n) as CSR (offsets_host [n + 1] from 0, terms_host, weights_host;
 *    any order within a row, empty rows allowed; the library sorts each row on the host) under the APPEND-ONLY rules of
 *    css_index_set_terms: with T the leading rows that have vectors, row0 == T appends, row0 < T first drops the vectors
 *    of ALL rows >= row0, row0 > T and a range outside [0, ntotal) are CSS_ERR_INVALID.  Offsets that do not start at 0
 *    or that decrease, a row of too many entries, a term >= 2^24, a weight that is NaN, infinite, zero, negative or too
 *    large, and a term repeated within a row are CSS_ERR_INVALID; the message names the row; all of it is checked before
 *    anything is written.  css_index_get_sparse reads the stored form of rows [row0, row0 + n) back: offsets_out
 *    [n + 1] from 0, then terms and weights (either may be NULL: a first call sizes the second).  css_index_sparse_rows
 *    gives T.
 *  - Storage.  Nothing is allocated before the first css_index_set_sparse.  Then 8 bytes per entry and 8 per row with
 *    a vector, the row offsets mirrored on the host.  NO df table and NO lengths: a dot product needs no corpus
 *    statistics, which also makes a shard's column equal to the single index's by construction.  The vectors follow
 *    the rows: kept through capacity growth, none for appended rows, forgotten by css_index_reset, compacted by
 *    css_index_remove_rows with the same keep bits -- afterwards css_index_get_sparse equals that of a fresh index built
 *    from the kept rows.
 *  - The column.  With the query's m <= CSS_MAX_SPARSE_QUERY_TERMS distinct terms t_j and weights w_j (finite, nonzero,
 *    |w_j| <= CSS_MAX_SPARSE_WEIGHT; negative weights are allowed), in fp32 and in this order (-ffp-contract=off):
 *        sp_r = 0.0f;  hit_r = false;
 *        for j = 0 .. m-1 in the caller's order:
 *            if row r stores t_j with weight d:  sp_r = sp_r + w_j * d;  hit_r = true;
 *        col[r] = hit_r ? sp_r : miss          // miss = 0.0f (hybrid) or -inf (pure sparse search); rows >= T: miss
 *    The sum runs in QUERY-TERM order, whatever the order of the entries in memory, so a float32 restatement gives the
 *    same bits and a shard gives the same bits as one index.
 *  - css_index_search_sparse.  One request per call, 1 <= k <= 128.  The k best HIT rows -- rows that share at least one
 *    term with the query -- among the allowed rows (allow_bits_host as in css_index_search_masked), ranked by the
 *    column ALONE: larger sp is better on an index of either metric, ties to the lower id (a hit row whose products
 *    cancel to 0.0 is still a hit).  D = sp, I = global ids.  Fewer than k hits, m == 0, an index without vectors or
 *    an empty index give padding: I = -1, D = -FLT_MAX.  On the device: k_sparse_scores with miss = -inf (8 bytes per
 *    entry and 8 per row read, 4 per row written), k_sparse_topk over slices of the column, the part merge.  No dense
 *    row is read.  One upload, one wait; a search never edits the index.
 *  - css_index_search_hybrid_sparse is css_index_search_hybrid with sp in the place of the BM25 column (miss = 0.0f):
 *        inner product   f = fmaf(alpha, sp_r, s)        larger is better
 *        squared L2      f = fmaf(-alpha, sp_r, dist)    smaller is better
 *    D, I, S, L (= sp of the returned rows) and the padding as there.  m == 0, alpha == 0 or an index without vectors
 *    give css_index_search_prior on an index without priors bit for bit. */
#define CSS_MAX_SPARSE_QUERY_TERMS 64
#define CSS_MAX_SPARSE_ROW_ENTRIES 65536
#define CSS_MAX_SPARSE_WEIGHT 65536.0f
int css_index_set_sparse(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host /* [n+1] */,
                         const uint32_t* terms_host, const float* weights_host);
int css_index_get_sparse(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out /* [n+1], from 0 */,
                         uint32_t* terms_out /* may be NULL */, float* weights_out /* may be NULL */);
int css_index_sparse_rows(css_index* ix, int64_t* rows_out);
int css_index_search_sparse(css_index* ix, const uint32_t* terms_host, const float* weights_host, int m, int k,
                            const uint32_t* allow_bits_host, float* D_host /* [k] */, int64_t* I_host /* [k] */);
int css_index_search_hybrid_sparse(css_index* ix, const float* q_host /* [dim] */, int k, float alpha,
                                   const uint32_t* terms_host, const float* weights_host, int m, int normalize_q,
                                   const uint32_t* allow_bits_host, float* D_host, int64_t* I_host,
                                   float* S_host /* may be NULL */, float* L_host /* may be NULL */);

/* Per-row token matrices and MaxSim search (late interaction as a FIRST stage and as a re-rank stage without a forward
 * pass: brute-force ColBERT, Vespa and Qdrant multi-vector, PyLate's index).  A row may carry a matrix of m token
 * vectors of P bf16 components each, such as css_encoder_forward_tokens produces; a query is such a matrix too.  A third
 * per-row list kind, independent of the term lists and the sparse vectors above: an index may carry any of them.
 *  - Matrices.  P is a multiple of 32 in [32, CSS_MAX_TOKEN_DIM]; the first call fixes it, a later call with another P
 *    is CSS_ERR_INVALID unless it rewrites from row0 == 0 (a call without rows only truncates: its P is not looked
 *    at).  At most CSS_MAX_ROW_TOKEN_VECTORS tokens per row; empty rows are
 *    allowed (a tombstone, a text whose every token was on the skiplist).  ColBERT's keep flags are applied BEFORE
 *    storing: a dropped token is not stored, and there are no flags here.  css_index_set_tokens takes rows
 *    [row0, row0 + n) as CSR (offsets_host [n + 1] from 0, in tokens; tok_host bf16 [offsets[n], P]) under the
 *    APPEND-ONLY rules of css_index_set_sparse: with T the leading rows that have matrices, row0 == T appends,
 *    row0 < T first drops the matrices of ALL rows >= row0, row0 > T and a range outside [0, ntotal) are
 *    CSS_ERR_INVALID.  Offsets that do not start at 0 or that decrease, a row of too many tokens and a NaN or infinite
 *    component are CSS_ERR_INVALID; the message names the row; all of it is checked before anything is written.
 *    css_index_get_tokens reads rows [row0, row0 + n) back: offsets_out [n + 1] from 0, then the tokens (tok_out may be
 *    NULL: a first call sizes the second).  css_index_token_rows gives T, css_index_token_dim gives P (0 while T == 0),
 *    css_index_drop_tokens drops the matrices and frees their memory.
 *  - Storage.  Nothing is allocated before the first css_index_set_tokens.  Then 2 P bytes per token and 8 per row
 *    with a matrix, the row offsets mirrored on the host.  The matrices follow the rows: kept through capacity growth,
 *    none for appended rows, forgotten by css_index_reset, compacted by css_index_remove_rows with the same keep bits --
 *    afterwards css_index_get_tokens equals that of a fresh index built from the kept rows.
 *  - The score.  For a query q [mq, P] bf16, 1 <= mq <= CSS_MAX_QUERY_TOKENS, finite components, and a row with
 *    md >= 1 stored tokens d_t:
 *        score = sum over s = 0 .. mq-1 (ascending, fp32) of  max over t of  dot(q_s, d_t)
 *    with bf16 operands and fp32 accumulation on v_mfma_f32_16x16x32_bf16, K steps of 32 in ascending order: exactly
 *    the value css_encoder_maxsim returns for the same bf16 rows with every token kept, bit for bit (the kernel keeps
 *    that kernel's operand roles and lane-to-k mapping), whatever the grid and whatever the shard.  A row >= T, an
 *    empty row and a masked row are a MISS: -inf in the column, never returned.
 *  - css_index_search_maxsim.  One request per call, 1 <= k <= 128; P is the query's width and must equal
 *    css_index_token_dim (any valid P while the index has no matrices).  The k best rows that are not a miss among the
 *    allowed rows (allow_bits_host as in css_index_search_masked; a masked row is skipped before any of its tokens is
 *    read), ranked by the score ALONE: larger is better on an index of either metric, ties to the lower id.
 *    D = score, I = global ids.  Fewer than k hits, an index without matrices or an empty index give padding: I = -1,
 *    D = -FLT_MAX.  On the device: k_tok_scores (2 P bytes per token of an allowed row read, 4 per row written),
 *    k_sparse_topk over slices of the column, the part merge.  No dense row is read.  One upload, one wait; a search
 *    never edits the index.
 *  - css_index_maxsim_rows.  The scores of the n <= CSS_MAX_MAXSIM_ROWS named rows (global ids, any order, repeats
 *    allowed), -inf for a row that is a miss: the re-rank stage without a forward pass.  An id outside the index is
 *    CSS_ERR_INVALID; the message names its position.  The same kernel through a row list.
 *  - css_index_set_token_blocks sets the grid of k_tok_scores (0: the library's choice -- resident blocks x CUs, and
 *    fewer than 16 rows per wave where the rows are few; a set grid always gives a wave 16 rows at a time), a diagnostic
 *    knob in the family of css_index_set_range_rows: the results do not depend on it. */
#define CSS_MAX_TOKEN_DIM 128
#define CSS_MAX_ROW_TOKEN_VECTORS 512   /* (CSS_MAX_ROW_TOKENS is the term lists' limit) */
#define CSS_MAX_QUERY_TOKENS 64
#define CSS_MAX_MAXSIM_ROWS 65536
int css_index_set_tokens(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host /* [n+1] */,
                         const uint16_t* tok_host /* bf16 [offsets[n], P] */, int P);
int css_index_get_tokens(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out /* [n+1], from 0 */,
                         uint16_t* tok_out /* may be NULL */);
int css_index_token_rows(css_index* ix, int64_t* rows_out);
int css_index_token_dim(css_index* ix, int* dim_out);
int css_index_drop_tokens(css_index* ix);
int css_index_set_token_blocks(css_index* ix, int blocks);
int css_index_search_maxsim(css_index* ix, const uint16_t* q_tok_host /* bf16 [mq, P] */, int mq, int P, int k,
                            const uint32_t* allow_bits_host, float* D_host /* [k] */, int64_t* I_host /* [k] */);
int css_index_maxsim_rows(css_index* ix, const uint16_t* q_tok_host /* bf16 [mq, P] */, int mq, int P,
                          const int64_t* ids_host /* [n] */, int64_t n, float* scores_out /* [n] */);

/* Compressed token matrices (ColBERTv2's residual compression): with a CODEC on the index a token is stored as the id
 * of its best centroid plus an nbits bucket per component for the residual -- 2 + P nbits / 8 bytes in place of 2 P
 * (34 in place of 256 at P = 128, nbits = 2) -- and MaxSim runs on the codes.  An index without a codec stores and
 * scores exactly as above.
 *  - The codec: C centroids [C, P], 1 <= C <= CSS_MAX_TOKEN_CENTROIDS, P a multiple of 32 in [32, CSS_MAX_TOKEN_DIM],
 *    every component a finite fp32 value that IS a bf16 value (its low 16 bits are zero; anything else is refused:
 *    rounding is the caller's decision); nbits in {1, 2, 4}; cutoffs [2^nbits - 1] fp32, finite and strictly ascending;
 *    weights [2^nbits] fp32, finite.
 *  - Encode, for a stored token d (bf16):  code = argmax over c of dot(d, centroid_c), ties to the lower c, the dot
 *    formed as the score's dots are (bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16, K steps of 32
 *    ascending);  r_j = fp32(d_j) - fp32(centroid[code]_j), one IEEE fp32 subtraction;  bucket_j = #{i : cutoffs[i] <
 *    r_j}  (np.searchsorted(cutoffs, r, side="left"), torch.bucketize).
 *  - Decode:  d'_j = bf16_rne(fp32(centroid[code]_j) + weights[bucket_j]), one fp32 addition and one rounding to nearest
 *    even.  There is NO renormalisation after decoding.  ColBERTv2 has one; it is left out so that a float32
 *    restatement (numpy) gives the same bytes, and so that the score below has one definition.
 *  - The score of a row is the score defined above of its DECODED matrix: bit for bit what css_encoder_maxsim returns
 *    for css_index_get_tokens of that row with every token kept.
 *  - Canonical code layout (what crosses this interface and goes to disk): codes uint16 [ntok]; res uint8
 *    [ntok, P nbits / 8]; component j's bucket sits in bits [nbits (j % (8 / nbits)), + nbits) of byte j nbits / 8, least
 *    significant first.
 *  - css_index_set_token_codec is allowed only while the index has no matrices (css_index_token_rows == 0), else
 *    CSS_ERR_INVALID; centroids_host == NULL clears the codec; everything is checked before anything is allocated.  The
 *    codec survives css_index_drop_tokens, css_index_reset and css_index_remove_rows, which drop or move matrices only.
 *    css_index_get_token_codec: any pointer may be NULL (sizes first, then contents); css_index_token_codec_bits: 0 =
 *    no codec.
 *  - With a codec, css_index_set_tokens takes the same CSR of bf16 matrices under the same rules and refusals, P must
 *    equal the codec's, and it compresses on the device (k_tok_encode) through a staging buffer that dies with the
 *    call: the raw tokens never stay in HBM.  css_index_get_tokens returns the DECODED matrices (k_tok_decode).
 *    css_index_get_token_codes / css_index_set_token_codes move canonical (offsets, codes, res) without encoding or
 *    decoding (save / load, shards); set follows the same append-only rules, needs a codec and refuses a code >= C,
 *    naming the row.  css_index_search_maxsim and css_index_maxsim_rows are unchanged in signature, limits, padding,
 *    masks, id_base and tie rule; on a compressed store they run k_tok_scores_c (2 + P nbits / 8 bytes per token of an
 *    allowed row read from HBM, the centroid table through the caches).  css_index_remove_rows compacts codes and
 *    packed buckets: afterwards css_index_get_token_codes equals that of a fresh index built from the kept rows. */
#define CSS_MAX_TOKEN_CENTROIDS 65536
int css_index_set_token_codec(css_index* ix, const float* centroids_host /* [C, P]; NULL clears */, int C, int P, int nbits,
                              const float* cutoffs_host /* [2^nbits - 1] */, const float* weights_host /* [2^nbits] */);
int css_index_get_token_codec(css_index* ix, int* C_out, int* P_out, int* nbits_out, float* centroids_out /* [C, P] */,
                              float* cutoffs_out, float* weights_out);
int css_index_token_codec_bits(css_index* ix, int* bits_out);
int css_index_get_token_codes(css_index* ix, int64_t row0, int64_t n, int64_t* offsets_out /* [n+1], from 0 */,
                              uint16_t* codes_out /* may be NULL */, uint8_t* res_out /* may be NULL */);
int css_index_set_token_codes(css_index* ix, int64_t row0, int64_t n, const int64_t* offsets_host /* [n+1] */,
                              const uint16_t* codes_host /* [offsets[n]] */, const uint8_t* res_host /* [offsets[n], P nbits / 8] */);

/* Candidate generation for MaxSim on a compressed store (PLAID's centroid interaction): rank every row by the MaxSim of
 * its tokens' CENTROIDS -- 2 bytes per token read and a small table -- and decode and score exactly only the best
 * ncand.  Both entry points need an index WITH a token codec (CSS_ERR_INVALID otherwise; the message says so), take
 * the query matrix of css_index_search_maxsim (the same checks) with P = the codec's P, and 1 <= ncand <=
 * CSS_MAX_MAXSIM_ROWS; everything is refused before anything is enqueued.  T, misses, masks and id_base as above.
 *  - The centroid table.  S[c, s] = dot(q_s, centroid_c), c < C, s < mq, formed exactly as the score's dot of query
 *    token s with a doc token equal to the bf16 centroid row c (bf16 operands, fp32 accumulation on
 *    v_mfma_f32_16x16x32_bf16, query tokens as rows of A, centroids as columns of B, K steps of 32 ascending).
 *  - The approximate score.  A[r] = sum over s ascending, fp32, of max over the row's tokens t of S[code_t, s]; a row
 *    >= T, an empty row and a masked row are a miss and never a candidate.  By construction A[r] is, bit for bit, the
 *    score defined above of the matrix centroids[codes of r]: what css_encoder_maxsim returns for those bf16 rows.
 *  - The candidates.  The first ncand rows of lexsort((id, -A)) among the rows that are no miss: A compared as floats
 *    (-0.0 == +0.0), ties to the lower id; fewer than ncand where fewer rows qualify.
 *  - css_index_maxsim_candidates returns them in ASCENDING id order with their A: *n_out <= ncand entries of ids_out
 *    and approx_out are written, the slots behind them are left alone.
 *  - css_index_search_maxsim_pruned.  The exact score of the candidates on the codes (k_tok_scores_c through its row
 *    list), then the k best by (score descending, id ascending), padded as css_index_search_maxsim pads; 1 <= k <=
 *    CSS_KERNEL_MAX_K, k <= ncand.  D is exactly css_index_maxsim_rows of I, and whenever ncand >= the number of
 *    allowed rows that are no miss the answer equals css_index_search_maxsim in bytes.  *ncand_out (may be NULL) = the
 *    number of candidates that were scored.
 *  - An index with a codec but no matrices returns no candidates and the padded answer.  On the device: k_tok_ctable,
 *    k_tok_ci (its grid follows css_index_set_token_blocks; no atomics, the bits do not depend on it), an exact
 *    multi-block radix select with an ordered compaction, k_tok_scores_c, k_sparse_topk and the part merge
 *    (css_token_prune.h), all on the index's stream: one upload, one wait; a call never edits the index. */
int css_index_maxsim_candidates(css_index* ix, const uint16_t* q_tok_host /* bf16 [mq, P] */, int mq, int P, int64_t ncand,
                                const uint32_t* allow_bits_host, int64_t* ids_out /* [ncand], global, ascending */,
                                float* approx_out /* [ncand] */, int64_t* n_out);
int css_index_search_maxsim_pruned(css_index* ix, const uint16_t* q_tok_host /* bf16 [mq, P] */, int mq, int P, int k,
                                   int64_t ncand, const uint32_t* allow_bits_host, float* D_host /* [k] */,
                                   int64_t* I_host /* [k] */, int64_t* ncand_out /* may be NULL */);

/* Batched MaxSim search: nq query matrices per call, the token store read once per GROUP of CSS_MAXSIM_BATCH_GROUP
 * queries instead of once per query.  The matrices lie one behind the other in q_tok_host: query b owns tokens
 * [q_offsets_host[b], q_offsets_host[b + 1]) (offsets from 0, ascending), all of one width P.
 *  - Limits.  1 <= nq <= CSS_MAX_MAXSIM_QUERIES, 1 <= k <= 128, every query 1 .. CSS_MAX_QUERY_TOKENS tokens with
 *    finite components, P as in css_index_search_maxsim.  allow_bits_host is ONE mask for all queries, as in
 *    css_index_search_masked.  A refusal names the offending query (and token) and comes before anything is enqueued.
 *  - Result.  Row b of D / I [nq, k] is, byte for byte, what css_index_search_maxsim returns for query b with the same
 *    k and mask: the score above, padding, id_base, rows >= T, empty rows, an index without matrices; on raw and on
 *    compressed stores.  The bits do not depend on the group a query falls into, on its slot, or on the grid.
 *  - On the device.  Per group of G queries: k_tok_scores_b (css_tokens_batch.h: a block of G waves, one query per
 *    wave, every 16-token tile loaded -- and on a compressed store decoded -- once per block and shared through LDS),
 *    k_sparse_topk over the G columns, ONE part merge for the G queries.  A group of one query (nq = 1, or a remainder
 *    of one) runs k_tok_scores / k_tok_scores_c as css_index_search_maxsim does.  Groups run back to back on the
 *    index's stream; the column workspace is G x rows x 4 bytes whatever nq.  One upload (offsets and matrices), one
 *    wait; the call never edits the index.  css_index_set_token_blocks sets the grid of k_tok_scores_b as well.
 *  - css_index_last_maxsim_passes: the scans of the store the last batch call made, ceil(nq / G); 0 when it returned
 *    padding without scanning (no matrices, no rows).  A diagnostic, as css_index_last_group_passes is. */
#define CSS_MAX_MAXSIM_QUERIES 1024
#define CSS_MAXSIM_BATCH_GROUP 8
int css_index_search_maxsim_batch(css_index* ix, const uint16_t* q_tok_host /* bf16 [q_offsets[nq], P] */,
                                  const int64_t* q_offsets_host /* [nq + 1], from 0 */, int nq, int P, int k,
                                  const uint32_t* allow_bits_host, float* D_host /* [nq, k] */, int64_t* I_host /* [nq, k] */);
int css_index_last_maxsim_passes(css_index* ix, int* passes_out);

/* MaxSim over per-query row lists, and the two-stage search built on it: a dense first stage whose best `fetch` rows
 * per query are re-ranked by MaxSim with the rows' stored matrices, in ONE call (Vespa's second phase, ColBERT as a
 * re-ranker).  The queries' matrices are given as in css_index_search_maxsim_batch (tokens, offsets from 0, one P), with
 * its limits and checks: 1 <= nq <= CSS_MAX_MAXSIM_QUERIES, every query 1 .. CSS_MAX_QUERY_TOKENS tokens with finite
 * components, P equal to css_index_token_dim (any valid P while the index has no matrices).  Every refusal names the
 * query, comes before anything is enqueued and leaves the index usable; neither call edits the index.
 *  - css_index_maxsim_rows_batch is css_index_maxsim_rows for nq queries, each with its own list of f ids, 1 <= f <=
 *    CSS_MAX_K: scores_out[b * f + j] has the bits of css_index_maxsim_rows(q_b, ids[b * f + j]), on raw and compressed
 *    stores, -inf for a miss.  Unlike the single call, an id outside the index is no refusal: it names no row and
 *    scores -inf (a list may carry the -1 padding of a search).  An index without matrices: all -inf.  One upload
 *    [offsets | row numbers | matrices], ONE launch of k_tok_scores_l (css_tokens_lists.h), one copy back, one wait.
 *  - css_index_search_rerank_maxsim.  q_host [nq, d] are the dense queries of the SAME nq requests; 1 <= fetch <=
 *    CSS_MAX_K, 1 <= k <= min(fetch, CSS_KERNEL_MAX_K); floor is a float, NaN = no floor.  Row b of the answer is:
 *    the pool (S0, I0) = css_index_search_masked(q_host, nq, fetch, normalize_q, allow_bits_host) of the same call
 *    shape; drop the entries with S0 < floor (that comparison on an index of either metric) and the -1 padding; score
 *    the rest with css_index_maxsim_rows(q_b, I0[b]); drop -inf; take the first k of a STABLE descending sort by that
 *    score -- ties keep the pool's order.  D [nq, k] = the MaxSim score, I = the global id, S = the row's dense score
 *    in the pool, R (int32) = its position in the pool.  Fewer than k entries, an index without matrices or without
 *    rows: padding, D = S = -FLT_MAX, I = R = -1.
 *    On the device, all on the index's stream under one turn at the workspaces: the pool search of css_index_search
 *    into owned lists, k_rr_lists (ids to row numbers under the floor), k_tok_scores_l, k_sparse_topk_cols over the
 *    [nq, fetch] columns by POSITION (one slice, no part merge) and k_rr_out.  One upload [dense queries | offsets |
 *    matrices], one wait; no id travels through the host.  css_index_set_token_blocks sets the grid of k_tok_scores_l
 *    as well; the bits do not depend on it, on nq or on a row's position in its list. */
int css_index_maxsim_rows_batch(css_index* ix, const uint16_t* q_tok_host /* bf16 [q_offsets[nq], P] */,
                                const int64_t* q_offsets_host /* [nq + 1], from 0 */, int nq, int P,
                                const int64_t* ids_host /* [nq, f] */, int f, float* scores_out /* [nq, f] */);
int css_index_search_rerank_maxsim(css_index* ix, const float* q_host /* [nq, d] */, int normalize_q,
                                   const uint16_t* q_tok_host /* bf16 [q_offsets[nq], P] */,
                                   const int64_t* q_offsets_host /* [nq + 1], from 0 */, int nq, int P, int fetch, int k,
                                   float floor, const uint32_t* allow_bits_host, float* D_host /* [nq, k] */,
                                   int64_t* I_host /* [nq, k] */, float* S_host /* [nq, k] */, int32_t* R_host /* [nq, k] */);

/* Significant terms (Elasticsearch's significant_terms aggregation, the keyword side of BERTopic): which terms set a
 * selection of rows apart from a background -- "what is in this cluster / this project / these hits".  Everything is
 * read from the term lists above; the rows' values play no part.  T = the leading rows that have lists.
 *  - Sets.  The selection S = {r < T : bit r of allow_bits_host} and the background B = {r < T : bit r of
 *    background_bits_host}, bitmaps as in css_index_search_masked over LOCAL rows; NULL means every row below T.  S must
 *    lie within B: otherwise CSS_ERR_INVALID, the message names the first offending row and nothing is written.
 *  - Counts.  fg[t] = the rows of S whose list holds term t, bg[t] the same for B (without a background mask that is
 *    the standing df table), FG = |S|, BG = |B|; rows with an empty list count in FG and BG.  Exact integers.
 *  - css_index_subset_terms: every term with fg >= 1, ascending by term, with its fg -- the form that shards exchange.
 *    Two-call sizing: *n_out = the number of such terms and *rows_out = FG always; the pairs are written when
 *    cap >= *n_out (terms_out, fg_out: cap entries each) and nothing is written when it is not (cap = 0: sizing).
 *  - css_index_significant_terms.  A term qualifies iff fg >= min_count (min_count >= 1) and fg * BG > bg * FG, compared
 *    in exact unsigned 64-bit integers.  Its score is JLH in float64, one IEEE rounding per operation, no contraction:
 *        p = (double)fg / (double)FG;   q = (double)bg / (double)BG;   score = (p - q) * (p / q);
 *    so a float64 restatement (lexical.significant_from_counts) gives the same bits.  The answer is the best m
 *    qualifying terms, 1 <= m <= CSS_MAX_SIG_TERMS, score descending, ties to the smaller term; *n_out <= m says how
 *    many qualified.  All m slots of terms_out / fg_out / bg_out / score_out are written: unused slots hold term
 *    0xFFFFFFFF, counts 0 and score 0.0.  *fg_rows_out = FG, *bg_rows_out = BG.
 *  - An index without lists, or an empty selection: *n_out = 0 and FG = BG = 0; no device is touched.
 *  - On the device (css_sigterms.h): one scatter-count over the lists of the selected rows into a zeroed uint32 table
 *    [2^24] (a second one under a background mask) with integer atomics only, a wave passing over 64 unselected rows
 *    for the price of their two mask words; one pass over the 2^24 slots qualifies and scores; an exact radix select on
 *    the 88-bit key (score bits, term) and a sort of the m winners.  The tables (64 MB each) and the candidate list are
 *    workspaces of the index, allocated on first use; they are not index state and outlive css_index_reset.  Locking
 *    and the call frame are those of css_index_term_stats; css_index_significant_terms waits for the device once,
 *    css_index_subset_terms twice when it writes.  Neither edits the index: df, the lists and every search are
 *    unchanged by them.
 *  - css_index_set_sigterm_slots: the (term, count) slots of the per-block LDS table in which the counting pass merges
 *    repeats of a term before it touches the global table (a term present in most rows would otherwise send one global
 *    add per row to one address).  -1 = the library's rule (4096), 0 = no table: every entry is one global add; else a
 *    power of two in [16, 4096].  A verification knob like css_index_set_gram_rows: the integers do not depend on it. */
#define CSS_MAX_SIG_TERMS 256
int css_index_set_sigterm_slots(css_index* ix, int slots);
int css_index_subset_terms(css_index* ix, const uint32_t* allow_bits_host, int64_t cap, uint32_t* terms_out /* [cap] */,
                           int64_t* fg_out /* [cap] */, int64_t* n_out, int64_t* rows_out);
int css_index_significant_terms(css_index* ix, const uint32_t* allow_bits_host,
                                const uint32_t* background_bits_host /* or NULL */, int m, int64_t min_count,
                                uint32_t* terms_out /* [m] */, int64_t* fg_out /* [m] */, int64_t* bg_out /* [m] */,
                                double* score_out /* [m] */, int* n_out, int64_t* fg_rows_out, int64_t* bg_rows_out);

/* Rows by id (faiss reconstruct_batch): the stored fp32 rows of the n GLOBAL ids (id_base included), gathered on the
 * device, as [n, dim] floats exactly as they lie in device memory.  Repeated ids are allowed.  An id outside
 * [id_base, id_base + ntotal) is CSS_ERR_INVALID: the message names it and nothing is enqueued.  n == 0 is a no-op.
 * Locking and the ordering behind asynchronous adds are those of css_index_search_rows. */
int css_index_export_rows(css_index* ix, const int64_t* ids_host, int64_t n, float* x_out_host);

/* One Lloyd step of k-means over the rows of the index ("what is in here": topics, a coarse quantiser): every allowed
 * row is assigned to its nearest centroid and the members of every centroid are summed, on the device.  The loop, the
 * initialisation and the empty-cluster rule are the caller's (flat_index.run_kmeans); this call is deterministic, so
 * they are too.
 *  - Assignment.  The metric is ALWAYS the squared L2 distance to the centroid, whatever the metric of the index (on
 *    unit rows and unit centroids that is the inner-product order).  Row r whose allow bit is set (allow_bits_host as
 *    in css_index_search_masked; NULL: every row) gets a(r) = argmax over c of key(r, c) = fmaf(-0.5f, ||c||^2,
 *    <x_r, c>), ties to the LOWER centroid index.  <x_r, c> is formed on the fp32-input matrix core
 *    (v_mfma_f32_32x32x2_f32, as the CSS_SEARCH_EXACT_FP32 scan of batches forms its scores): fp32 products, fp32
 *    accumulation over the padded row.  ||c||^2 is formed once per call in fp32 from the uploaded table.  No
 *    reduced-precision copy of the rows takes part, and the search mode plays none.
 *  - Distance.  dist(r) = fmaxf(0, fmaf(-2, key(r, a(r)), xnorm2[r])) with the squared row norms the index keeps.
 *  - Rows that are not allowed: assign = -1, dist = 0; they count nowhere.
 *  - Sums are fixed point.  sums[c][j] = sum over a(r) = c of llrint(x_r[j] * 2^s) as int64 (round to nearest even),
 *    counts[c] = the number of members, obj = sum over allowed r of llrint(dist(r) * 2^t).  They are exact integers:
 *    identical from run to run and for any grid shape, and shards that use one s add up to the unsharded values.
 *  - The shift rule (flat_index.kmeans_shift restates it).  ex = frexp(max_norm2) exponent with max_norm2 the running
 *    maximum of ||row||^2 (css_index_bounds [0]), ex = 0 when that is 0; e = ceil(ex / 2), so every |x| < 2^e;
 *    b = bit_length(max(ntotal, 1) - 1); s = 62 - b - e; t = s - e - 2.  n * 2^(s + e) <= 2^62: no sum reaches 2^63.
 *    (obj assumes dist < 2^(2e + 2), i.e. centroids no longer than the longest row, which holds for means of rows; it
 *    wraps, as int64, for centroids far outside the data.)
 *  - fx_shift < 0: the library chooses s by the rule.  fx_shift >= 0 imposes s (a sharded index passes the s of the
 *    global row count and the global maximum); a value above what this index's own ntotal and maximum can hold is
 *    CSS_ERR_INVALID and the message names the largest safe value.  *fx_shift_used = s, *obj_shift_used = t (either
 *    may be NULL).
 *  - 2 <= nc <= CSS_MAX_CENTROIDS, anything else is CSS_ERR_INVALID.  A centroid component that is NaN or infinite is
 *    CSS_ERR_INVALID: the message names the centroid and nothing is enqueued.  An empty index gives zero sums, counts
 *    and obj.  Rows are assumed finite: what a NaN or infinite row does to the result is NOT defined (nothing is read or
 *    written out of bounds).
 *  - sums_host [nc, dim], counts_host [nc], obj_host [1] are always written; assign_host (int32 [ntotal]) and dist_host
 *    (float [ntotal]) may be NULL, and are in LOCAL row numbering.
 *  - Locking, the ordering behind asynchronous adds and the call frame are those of css_index_search_prior; the call
 *    waits for the device once.  Its workspaces (centroid table, assign / dist, member lists, sums) belong to the index,
 *    grow on demand and outlive css_index_add, css_index_remove_rows and css_index_reset.
 *  - On the device: the assignment (128 rows x 128 centroids per tile; a lane holds the scores of one row, so the
 *    argmax is a register reduction), an exclusive scan of the counts, member lists appended through one cursor per
 *    centroid, and one block per (centroid, 1024 members) that sums llrint(x * 2^s) in int64 registers and flushes one
 *    64-bit integer atomic per column.  No float atomics, no sort. */
#define CSS_MAX_CENTROIDS 4096
int css_index_kmeans_step(css_index* ix, const float* centroids_host /* [nc, dim] */, int nc,
                          int fx_shift /* < 0: chosen by the library */, const uint32_t* allow_bits_host,
                          int64_t* sums_host /* [nc, dim] */, int64_t* counts_host /* [nc] */,
                          int64_t* obj_host /* [1] */, int* fx_shift_used, int* obj_shift_used,
                          int32_t* assign_host /* [ntotal], may be NULL */,
                          float* dist_host /* [ntotal], may be NULL */);

/* The second-moment (Gram) matrix X^T X of the stored rows with their column sums, in fixed point, on the device: the
 * reduction PCA needs (flat_index.pca_from_gram turns it into mean, covariance and components on the host), without
 * the rows leaving HBM.  k-means' sibling: one deterministic primitive here, the eigen-solve and the policy in Python.
 *  - Quantisation.  For every allowed row r (allow_bits_host as in css_index_search_masked; NULL: every row)
 *    q_r[j] = llrint((double)x_r[j] * 2^p): an exact float64 scaling, then round to nearest even.
 *  - Outputs.  gram[i][j] = sum over r of q_r[i] * q_r[j] (the full symmetric [dim, dim] matrix; pad columns never
 *    appear), colsum[j] = sum over r of q_r[j], count = the number of allowed rows.  They are exact integers: the same
 *    bytes on every run and for any grid shape, and shards that use one p add up to the unsharded values.
 *  - The shift rule (flat_index.pca_shift restates it).  ex, e and b exactly as in css_index_kmeans_step: ex = frexp
 *    exponent of the running maximum of ||row||^2 (0 when that is 0), e = ceil(ex / 2) so that every |x| < 2^e,
 *    b = bit_length(max(ntotal, 1) - 1).  p = min(20, (62 - b) >> 1) - e.  Hence |q| <= 2^(p + e) <= 2^20, a product is
 *    at most 2^40 and ntotal * 2^(2 (p + e)) <= 2^62: no sum reaches 2^63.  b uses ntotal, not the allowed count, so the
 *    rule does not depend on the mask.  Unit rows have e = 1: up to 2^22 of them give p = 19, 10 M give p = 18.
 *  - fx_shift < 0: the library chooses p by the rule.  fx_shift >= 0 imposes p (a sharded index passes the p of the
 *    global row count and the global maximum); a value above what this index's own ntotal and maximum can hold is
 *    CSS_ERR_INVALID and the message names the largest safe value.  *fx_shift_used = p (may be NULL).  The rule is
 *    evaluated on the device; the call waits for the device once.  The rule's own p is negative for rows longer
 *    than 2^20; a NEGATIVE p cannot be imposed (the sign means "choose"), so shards of such rows cannot be combined.
 *  - An empty index, or a mask that allows nothing, gives zeros.  Rows are assumed finite: what a NaN or infinite row
 *    does to the result is NOT defined (nothing is read or written out of bounds).
 *  - Locking, the ordering behind asynchronous adds and the call frame are those of css_index_kmeans_step.  The
 *    workspace belongs to the index, grows on demand and outlives css_index_add, css_index_remove_rows and
 *    css_index_reset.
 *  - On the device: the fp64 matrix core (v_mfma_f64_16x16x4_f64) with the rows as the K dimension, one 128 x 128 tile
 *    of the upper triangle and one strip of rows per block.  |q| <= 2^20 makes a partial sum over at most 8192 rows an
 *    integer of at most 2^53, which fp64 accumulates exactly in any order; every 8192 rows the accumulators are folded
 *    into int64 registers, and a block flushes once with 64-bit integer atomics.  No float atomics. */
/* Rows per block of the Gram kernel (0 = the library's rule: about four blocks per CU, at least 512 rows).  A
 * verification knob like css_index_set_range_rows: the integers of css_index_gram do not depend on it.  Values above
 * 8192 make a block fold its fp64 accumulators into int64 more than once. */
int css_index_set_gram_rows(css_index* ix, int64_t rows);
int css_index_gram(css_index* ix, int fx_shift /* < 0: chosen by the library */, const uint32_t* allow_bits_host,
                   int64_t* gram_host /* [dim, dim] */, int64_t* colsum_host /* [dim] */, int64_t* count_host /* [1] */,
                   int* fx_shift_used);

/* A linear transform of stored rows (faiss' LinearTransform / PCAMatrix apply, a 2-D map, a reduced copy, whitening):
 * y[r][c] = (sum over j of x_r[j] * A[c][j]) + b[c] for the rows r in [row0, row0 + n), LOCAL row numbering, range-checked
 * like css_index_export; n == 0 is a no-op.  1 <= m <= CSS_MAX_TRANSFORM_ROWS, anything else is CSS_ERR_INVALID.  A
 * non-finite entry of A or b is CSS_ERR_INVALID: the message names it and nothing is enqueued.  b_host NULL means b = 0.
 *  - Products and accumulation run in fp32 on the fp32-input matrix core (v_mfma_f32_32x32x2_f32) over the padded row,
 *    as css_index_kmeans_step forms its scores, with A in the place of the centroid table; b[c] is added once, in
 *    fp32.  No reduced-precision copy of the rows takes part, and the search mode plays none.
 *  - Tombstoned rows are transformed like any other: the caller selects.
 *  - Locking, the ordering behind asynchronous adds and the call frame are those of css_index_kmeans_step; the call
 *    waits for the device once.  Results come back in batches of rows through a workspace of the index. */
#define CSS_MAX_TRANSFORM_ROWS 256
int css_index_transform(css_index* ix, const float* A_host /* [m, dim] */, const float* b_host /* [m] or NULL */, int m,
                        int64_t row0, int64_t n, float* y_out_host /* [n, m] */);

/* Diversified search (maximal marginal relevance, MMR; langchain's max_marginal_relevance_search, the "diversity"
 * option of vector stores): k rows picked greedily from a pool of the best rows, each pick trading its score against
 * its similarity to the rows already picked -- so near-copies of one passage do not fill the answer.  Per query, with
 * m = fetch and the weight lam in [0, 1]:
 *  1. Candidates.  The ordinary ranked, masked search for m rows (what css_index_search_masked returns for k = m: search
 *     mode, reduced-precision copies, mask as there): a best-first list (s_c, id_c), c = 0 .. m'-1, of m' <= m valid
 *     entries with the pads at the tail.
 *  2. Relevance.  rel_c = s_c for the inner product, rel_c = -s_c for L2.
 *  3. Similarity.  sim(a, b) is formed in fp32 from the STORED fp32 rows, never from the bf16 or int8 copies:
 *     <x_a, x_b> for the inner product; -||x_a - x_b||^2 for L2, summed as squared differences (so copies of a row give
 *     exactly 0; norms minus twice the product would not).
 *  4. Picks.  p_0 = 0.  For t >= 1: pen_c = max over u < t of sim(c, p_u), v_c = lam * rel_c - (1 - lam) * pen_c in fp32
 *     (two products and a difference, each rounded), and p_t is the unpicked valid c with the largest v_c; ties go to the
 *     smaller c, i.e. the better score, then the lower id.
 *  5. Output.  D[j, t] = s_{p_t}, I[j, t] = id_{p_t} for t < min(k, m'), in PICK order (not sorted by D), then padded
 *     like css_index_search (I = -1, D = -FLT_MAX / +FLT_MAX).  D is the ordinary query score, so thresholds keep their
 *     meaning.
 *  - lam = 1 picks the first k entries of the pool: what css_index_search_masked returns for k.  (A score's last bits
 *    depend on the kernel that formed it, which the search chooses by nq, k and the index size; D here carries the bits
 *    of the search for m rows.)  lam = 0 ignores the query beyond the choice of the pool.
 *  - Limits: 1 <= k <= fetch <= 128 (the kernels' list size).  fetch = 0 means automatic: 32 if 4k <= 32, otherwise 128
 *    -- the two list classes of the grouped search.  lam outside [0, 1] or NaN, and any other value of k or fetch, is
 *    CSS_ERR_INVALID; the message names the argument.
 *  - An empty index gives fully padded rows; nq == 0 is a no-op.  normalize_q, allow_bits, rows appended on other
 *    streams, the serialisation of the searches of one index and the shared workspaces are those of
 *    css_index_search_masked / _dev.
 *  - On the device: the pool search writes into lists the index owns ([nq, fetch]); then one 256-thread block per query
 *    keeps rel, pen and the candidates' rows in LDS, updates pen against the LAST pick only -- (k - 1) * m' row pairs
 *    are read in place per query, there is no gathered copy and no m x m matrix -- and closes every step with a
 *    block-wide argmax.  Nothing depends on a readback: the _dev form enqueues everything on `stream` and returns. */
int css_index_search_diverse(css_index* ix, const float* q_host, int64_t nq, int k, int fetch, float lam,
                             int normalize_q, const uint32_t* allow_bits_host, float* D_host, int64_t* I_host);
int css_index_search_diverse_dev(css_index* ix, const float* q_dev, int64_t nq, int k, int fetch, float lam,
                                 int normalize_q, const uint32_t* allow_bits_dev, float* D_dev, int64_t* I_dev,
                                 void* stream);

/* Range search (faiss IndexFlat::range_search): EVERY row with score > radius (inner product) / squared distance
 * < radius (L2) -- strict, faiss' comparison -- as a variable-length hit list behind a handle.
 *  - Query j's hits are D / I[lims[j] .. lims[j+1]), lims[0] = 0 (nq + 1 entries).  Ids are global (id_base added),
 *    int64, never -1, never repeated inside a query.  nq = 0 and an empty index give lims of zeros.
 *  - Order inside a query is defined (faiss leaves it open): best score first (IP descending, L2 ascending), equal
 *    scores by ascending id.  The sort runs on the HOST side of the library, per query segment, after the copy back
 *    (the device appends hits in whatever order its waves reach them).
 *  - Scores are formed by an exact fp32 sweep of the fp32 rows (fmaf chains over the padded row, the arithmetic of
 *    CSS_SEARCH_EXACT_FP32; L2 from differences, never negative).  The float compared with the radius is the float
 *    returned.  Nothing depends on the reduced-precision row copies (css_index_set_shadow) or on the search mode.
 *  - One sweep of the rows serves up to 16 queries; longer batches are walked 16 queries at a time (a correctness
 *    path, not a fast one).  A sweep counts every hit even where its device pool is too small; the pool is then grown
 *    to the counted size and the sweep repeated ONCE.
 *  - normalize_q, allow_bits_host (may be NULL), rows appended by css_index_add_dev / css_index_add_synthetic on other
 *    streams and the shared workspaces behave as for css_index_search_masked.  A NaN radius is CSS_ERR_INVALID.
 *  - If the counted result cannot be allocated (device pool or host memory) the call returns CSS_ERR_OOM with the hit
 *    count in the message; the index stays usable.  *out is NULL after every failure.
 *  - The handle owns host memory only and is complete when the call returns: it is independent of the index (which may
 *    be searched, changed or freed while the handle lives) and may be read from any thread.  css_range_result_lims
 *    writes nq + 1 entries, css_range_result_read lims[nq] entries each; css_range_result_free(NULL) is allowed. */
typedef struct css_range_result css_range_result;
int css_index_range_search(css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q,
                           const uint32_t* allow_bits_host, css_range_result** out);
int css_range_result_lims(const css_range_result* r, int64_t* lims_host);
int css_range_result_read(const css_range_result* r, float* D_host, int64_t* I_host);
int css_range_result_free(css_range_result* r);

/* Facet counts (Elasticsearch's terms / date_histogram aggregations, Qdrant's facet API, Vespa grouping): per query,
 * how many rows within the radius fall into each bucket of a per-row int32 column, and the best such row per bucket.
 * The reference answers "which projects / sessions exist" only without a query (get_stats, src/storage.py:654;
 * get_all_projects, :721), yet its search filters --project / --after / --before / --session (src/cli.py:338-342) can
 * only be set well after seeing where the matches of a query lie; this call is that distribution.
 *  - A row hits query j when score > radius (inner product) / squared distance < radius (L2): strict, NaN never, the
 *    predicate and the fp32 sweep of css_index_range_search -- a row hits here exactly when it hits there, with the
 *    same float.  Nothing depends on the reduced-precision row copies or on the search mode.
 *  - The bucket of row r is buckets_host[r] (a per-call column in LOCAL row numbering, uploaded on every call into a
 *    kept workspace, never stored) or, with buckets_host == NULL, the row's group label (css_index_set_groups; no
 *    upload).  A hit with bucket b in [0, nbuckets) counts in count_out[j * nbuckets + b]; every other hit (negative
 *    label, b >= nbuckets, or labels that were never set) counts in unbucketed_out[j] only; total_out[j] counts all
 *    hits: total = sum_b count + unbucketed.
 *  - best_score_out / best_id_out (either may be NULL): the best hit of the bucket -- best score, equal scores to the
 *    smallest id; ids are global (id_base added) as css_index_range_search's.  An empty bucket has count 0, id -1 and
 *    the score css_index_search pads with (-FLT_MAX inner product, +FLT_MAX L2).
 *  - Counts and keys are integers combined by atomic add and max only, so the answer is the same bytes on every run
 *    and whatever the placement of the table.  No hit list exists at any point: no pool, no second sweep, no sort.
 *  - One sweep of the rows serves min(16, the queries whose rows fit 64 KiB of LDS, 2^20 / nbuckets) queries; its
 *    table (at most 2^20 entries of 12 bytes) lives in a workspace of the index, is zeroed before and copied back
 *    after the sweep, and is decoded on the host side of the library.
 *  - nq in [0, 2^24); 1 <= nbuckets <= CSS_MAX_FACET_BUCKETS; a NaN radius is CSS_ERR_INVALID, +-inf is legal (IP
 *    radius -inf counts every allowed row); fewer than 2^32 - 1 rows.  nq == 0 writes nothing; an empty index answers
 *    zero counts and empty slots without a launch.  normalize_q, allow_bits_host (may be NULL), rows appended on other
 *    streams and the shared workspaces behave as for css_index_search_masked.  A failed allocation (table, column or
 *    host memory) is CSS_ERR_OOM and leaves the index as it was.
 *  - css_index_last_facet_sweeps: sweeps of the last call, and how many of them kept their table in LDS.
 *  - css_index_set_facet_lds_entries: the largest table (queries x buckets of one sweep) that goes to LDS; -1 (default)
 *    the library's rule, 0 never.  A table that does not fit the 160 KB of a CU beside the query rows
 *    goes to global memory whatever is set.  For measurements and tests; the answer does not depend on it. */
#define CSS_MAX_FACET_BUCKETS (1 << 20)
int css_index_facets(css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q,
                     const uint32_t* allow_bits_host, const int32_t* buckets_host, int64_t nbuckets, int64_t* count_out,
                     float* best_score_out, int64_t* best_id_out, int64_t* total_out, int64_t* unbucketed_out);
int css_index_last_facet_sweeps(css_index* ix, int64_t* sweeps, int64_t* lds_sweeps);
int css_index_set_facet_lds_entries(css_index* ix, int64_t entries);

/* Attribute columns and filters on the device (Qdrant payload indexes, Milvus scalar filtering, Vespa attributes,
 * Elasticsearch filter context).  The reference filters AFTER the search, one chunk at a time in Python
 * (_matches_filters, src/storage.py:508-543: project_name, has_code, session_id, a timestamp range); every search
 * here takes an allow bitmap instead, and these calls produce that bitmap from values kept beside the rows.
 *  - Columns.  CSS_MAX_ATTRS numbered slots, each one 4-byte value per row in LOCAL row numbering, typed
 *    CSS_ATTR_I32 or CSS_ATTR_F32 by its first css_index_set_attr with n > 0; a later set with the other type is
 *    CSS_ERR_INVALID and names the slot.  A slot that was never set holds no memory.  Rows never given a value, and rows
 *    appended after a set, hold the default: every byte 0xFF, i.e. -1 (int32) / a NaN (float32).  The columns follow
 *    the rows like the group labels: kept through capacity growth, compacted by css_index_remove_rows with the same
 *    keep bits, forgotten (values AND types) by css_index_reset.  css_index_get_attr reads rows [row0, row0 + n) back
 *    as stored (an unset slot answers the default bytes); css_index_attr_type gives the type, -1 for an unset slot;
 *    css_index_drop_attr frees a slot and forgets its type (an unset slot: nothing happens).  Locking and the wait on
 *    pending asynchronous adds are those of css_index_set_groups / css_index_get_groups.  Values are stored as given:
 *    no range or NaN check.
 *  - css_index_where.  bits_out_host [ceil(ntotal / 32)] receives bit r & 31 of word r >> 5 = 1 exactly when row r
 *    passes ALL nclauses clauses and, with allow_bits_host given, its allow bit is set; the bits of the last word past
 *    ntotal are zero and nothing past the last word is written.  *count_out is the number of set bits.  nclauses == 0
 *    answers the allow bits (or all rows) cut to ntotal.  An empty index writes nothing and counts 0.
 *  - A css_clause compares the value of row r in `slot` with the operand: EQ NE LT LE GT GE compare with `value`
 *    (an int32, or the BITS of a float32 for a float slot) exactly as numpy compares int32 / float32 arrays: a NaN, stored
 *    or as operand, fails every op except NE; -0.0 == 0.0; denormals compare as themselves (the device compares
 *    ordered integer keys, so the denormal mode of the build does not matter).  IN / NOT_IN are for int32 slots only:
 *    the operand is a bit table over [0, table_bits), table_bits <= CSS_MAX_TABLE_BITS, that starts at WORD table_off of
 *    tables_host [table_words]; bit v & 31 of word table_off + (v >> 5) says whether v is in.  A stored value that is
 *    negative or >= table_bits is "not in" (so the default -1 passes NOT_IN and fails IN).  Tables of several clauses may
 *    overlap.  All tables of a call go to LDS when table_words <= 8192 (32 KiB) and are read from global memory (L2)
 *    otherwise; the answer does not depend on it.
 *  - CSS_ERR_INVALID, with nothing enqueued and nothing written: nclauses outside [0, CSS_MAX_CLAUSES]; a slot outside
 *    [0, CSS_MAX_ATTRS); a clause on a slot that was never set (the message names the slot); an unknown op; IN / NOT_IN
 *    on a float slot; a table that does not lie inside tables_host or has more than CSS_MAX_TABLE_BITS bits.
 *  - The count is a sum of integers (one atomic add per block), so the answer is the same bytes on every call.  The
 *    call runs on the index's own stream inside the frame of the host searches (allow bitmap up, result through
 *    pinned staging when it is small); rows appended on other streams have landed before it reads.  There is no _dev
 *    form: the bitmap goes back to the host and into the allow argument of any search.
 *  - css_index_facets_attr is css_index_facets with the int32 attribute column `slot` as the bucket column: nothing
 *    is uploaded.  A float or unset slot is CSS_ERR_INVALID. */
#define CSS_MAX_ATTRS 16
#define CSS_MAX_CLAUSES 16
#define CSS_MAX_TABLE_BITS (1 << 27)
enum { CSS_ATTR_I32 = 0, CSS_ATTR_F32 = 1 };
enum { CSS_WHERE_EQ = 0, CSS_WHERE_NE = 1, CSS_WHERE_LT = 2, CSS_WHERE_LE = 3, CSS_WHERE_GT = 4, CSS_WHERE_GE = 5,
       CSS_WHERE_IN = 6, CSS_WHERE_NOT_IN = 7 };
typedef struct css_clause {
    int32_t slot;
    int32_t op;
    int32_t value;        /* EQ .. GE: the int32 operand, or the bits of the float32 operand */
    int32_t reserved;     /* 0 */
    int64_t table_off;    /* IN / NOT_IN: first word of the table in tables_host */
    int64_t table_bits;   /* IN / NOT_IN: bits of the table */
} css_clause;
int css_index_set_attr(css_index* ix, int slot, int type, int64_t row0, int64_t n, const void* values_host);
int css_index_get_attr(css_index* ix, int slot, int64_t row0, int64_t n, void* out_host);
int css_index_attr_type(css_index* ix, int slot, int* type);
int css_index_drop_attr(css_index* ix, int slot);
int css_index_where(css_index* ix, const css_clause* clauses, int nclauses, const uint32_t* tables_host,
                    int64_t table_words, const uint32_t* allow_bits_host, uint32_t* bits_out_host, int64_t* count_out);
int css_index_facets_attr(css_index* ix, const float* q_host, int64_t nq, float radius, int normalize_q,
                          const uint32_t* allow_bits_host, int slot, int64_t nbuckets, int64_t* count_out,
                          float* best_score_out, int64_t* best_id_out, int64_t* total_out, int64_t* unbucketed_out);

/* Merge `nparts` per-shard results ([nparts, nq, k] each) into the global
 * top-k by (score, id); used after the RCCL all-gather of per-shard top-k. */
int css_merge_topk_dev(const float* D_parts_dev, const int64_t* I_parts_dev, int nparts,
                       int64_t nq, int k, int metric, float* D_out_dev, int64_t* I_out_dev,
                       int device, void* stream);

/* The same merge straight from the exchange buffer of the sharded search: `nparts` records of `record_bytes`
 * bytes (a multiple of 8, >= 12 * nq * k), each [nq * k int64 ids][nq * k float scores] -- the layout one
 * RCCL all-gather of nq * k * 12 bytes per rank produces (a single exchange step). */
int css_merge_topk_packed_dev(const void* packed_dev, int nparts, int64_t record_bytes, int64_t nq, int k,
                              int metric, float* D_out_dev, int64_t* I_out_dev, int device, void* stream);

/* ---- sentence encoder: MPNet (all-mpnet-base-v2 architecture) or BERT ---- */
#define CSS_ENCODER_ARCH_MPNET 0
#define CSS_ENCODER_ARCH_BERT 1
#define CSS_ENCODER_POOL_MEAN 0
#define CSS_ENCODER_POOL_CLS 1
typedef struct css_encoder_cfg {
    int num_layers;       /* 12 */
    int hidden;           /* 768 (BERT: 384 or 768) */
    int heads;            /* 12 (head_dim = hidden / heads: 64; BERT: 32 at hidden 384, 64 at hidden 768) */
    int ffn;              /* 3072 */
    int vocab;            /* 30527 */
    int max_pos;          /* 514 */
    int rel_buckets;      /* 32 */
    int pad_id;           /* 1 */
    int max_seq_len;      /* 384 (kernel limit 512) */
    float ln_eps;         /* 1e-5 */
    int compute;          /* 0 = bf16 MFMA (product), 1 = fp32 verification mode */
    /* Trailing fields: 0 keeps the MPNet / mean-pooling meaning of a zeroed or shorter-initialised struct. */
    int arch;             /* CSS_ENCODER_ARCH_MPNET (0) or CSS_ENCODER_ARCH_BERT (1): BERT = absolute positions 0..L-1
                             plus token_type_embeddings row 0, no relative bias, tensor names of transformers' BertModel
                             (max_pos >= max_seq_len, rel_buckets ignored, 2 token types) */
    int pooling;          /* CSS_ENCODER_POOL_MEAN (0): masked mean of the token rows; CSS_ENCODER_POOL_CLS (1): row of
                             token 0 of every sequence */
} css_encoder_cfg;

typedef struct css_tensor {
    const char* name;     /* HF key, e.g. "encoder.layer.0.attention.attn.q.weight" */
    const float* data;    /* host fp32, row-major */
    int64_t numel;
} css_tensor;

/* css_encoder_create refuses (CSS_ERR_INVALID) a geometry the kernels are not built for: hidden / heads (comments
 * above), ffn no multiple of 128, num_layers outside [1, 64], max_seq_len outside [1, 512], max_pos too small for
 * max_seq_len, vocab < 1, pad_id outside the vocabulary, MPNet rel_buckets no positive multiple of 4, compute not 0 / 1.
 * vocab may be as small as 1 (the masked-LM head's vocabulary maximum is defined for any V >= 1); ids are checked
 * against it on every call. */
int css_encoder_create(const css_encoder_cfg* cfg, int device, css_encoder** out);
int css_encoder_free(css_encoder* enc);
int css_encoder_load_weights(css_encoder* enc, const css_tensor* tensors, int n);
/* Seeded synthetic weights generated on the device ("synthetic weights"). */
int css_encoder_init_synthetic(css_encoder* enc, uint64_t seed);
/* Copy one named parameter (fp32 master copy) back to the host. */
int css_encoder_export_weight(const css_encoder* enc, const char* name, float* out_host, int64_t numel);
/* Packed var-len batch: input_ids[cu_seqlens[B]] tokens, sequence b occupies
 * [cu_seqlens[b], cu_seqlens[b+1]); every length in [1, max_seq_len].
 * out: [B, hidden] fp32 = masked mean-pool or CLS row (cfg.pooling) (+ L2 normalise when normalize != 0).
 * The same batch gives the same bits on every run (row statistics of the folded
 * LayerNorm are accumulated with integer atomics); another batch composition may take
 * another kernel path (GEMM tile walk, folded / separate LayerNorm): bf16 rounding noise. */
int css_encoder_forward(css_encoder* enc, const int32_t* input_ids_host, const int32_t* cu_seqlens_host,
                        int B, int normalize, float* out_host);
int css_encoder_forward_dev(css_encoder* enc, const int32_t* input_ids_dev, const int32_t* cu_seqlens_dev,
                            int B, int total_tokens, int max_len, int normalize, float* out_dev, void* stream);

/* The forward pass of css_encoder_forward, plus one pooled row per SPAN of token rows (best passages of a search hit:
 * sentence vectors that have seen the whole chunk as context, from one forward pass).
 * spans: [S][3] int32 = (sequence b, begin, end), token positions relative to the sequence,
 * 0 <= begin < end <= len_b.  Spans may overlap, repeat, come in any order, and leave sequences uncovered.
 * span_out [S, hidden] (may be NULL): masked MEAN of the final hidden states of tokens begin..end-1
 *   (always the mean, also for a CLS-pooling model), then e / max(||e||, 1e-12) when normalize != 0.
 * q [hidden] (may be NULL) with scores_out [S] (NULL exactly when q is): dot(q, span row as written to span_out),
 *   formed on the device.
 * seq_out [B, hidden] (may be NULL): exactly what css_encoder_forward writes.
 * S == 0 is allowed.  A bad span fails before anything is enqueued, naming the span.  The same call gives the same
 * bits on every run (one block per span, fixed summation order).  The tiny-batch graphs of css_encoder_forward are
 * not used by this call, and growing its span buffers does not drop them.
 * _dev: device pointers, enqueued on `stream` without a synchronise.  The span table cannot be checked there: the
 * kernels clamp (b, begin, end) into the batch, so a bad span yields a meaningless row, never a read outside it. */
int css_encoder_forward_spans(css_encoder* enc, const int32_t* input_ids_host, const int32_t* cu_seqlens_host, int B,
                              const int32_t* spans_host, int S, const float* q_host, int normalize,
                              float* seq_out_host, float* span_out_host, float* scores_out_host);
int css_encoder_forward_spans_dev(css_encoder* enc, const int32_t* input_ids_dev, const int32_t* cu_seqlens_dev, int B,
                                  int total_tokens, int max_len, const int32_t* spans_dev, int S, const float* q_dev,
                                  int normalize, float* seq_out_dev, float* span_out_dev, float* scores_out_dev,
                                  void* stream);

/* ---- cross-encoder re-ranking: one relevance logit per (query, text) pair ----
 * Sequence-classification head of a BERT cross-encoder (transformers' BertForSequenceClassification, num_labels = 1):
 * pooled = tanh(Wp h_CLS + bp), logit = dot(wc, pooled) + bc.  Host fp32; copies are kept on the device.
 * Separate from css_encoder_load_weights (which still skips pooler.* and does not know classifier.*).  BERT
 * architecture only (anything else: CSS_ERR_INVALID).  May be called again to replace the head. */
int css_encoder_set_head(css_encoder* enc, const float* pooler_w /* [H,H] */, const float* pooler_b /* [H] */,
                         const float* cls_w /* [H] */, const float* cls_b /* [1] */);
/* Packed var-len batch as css_encoder_forward, plus seg_starts[b] in [1, len_b]: tokens at positions < seg_starts[b]
 * of sequence b take token type 0, the others type 1 (seg_starts[b] == len_b: a single-segment input).
 * logits_out [B] fp32: the head applied to the final hidden state of token 0 of every sequence (whatever cfg.pooling is).
 * The head is fp32 in both compute modes and uses no atomics: the same batch gives the same bits on every run.
 * A seg_start outside [1, len_b] fails before anything is enqueued, naming the sequence.  An MPNet encoder is
 * CSS_ERR_INVALID, an encoder without a head CSS_ERR_STATE.  The tiny-batch graphs of css_encoder_forward are not
 * used, created or dropped by this call (as for css_encoder_forward_spans).
 * _dev: device pointers, enqueued on `stream` without a synchronise.  seg_starts cannot be checked there: the kernels
 * clamp it into [1, len_b], so a bad value yields a meaningless logit, never a read outside the batch. */
int css_encoder_forward_pairs(css_encoder* enc, const int32_t* input_ids_host, const int32_t* cu_seqlens_host,
                              const int32_t* seg_starts_host, int B, float* logits_out_host);
int css_encoder_forward_pairs_dev(css_encoder* enc, const int32_t* input_ids_dev, const int32_t* cu_seqlens_dev,
                                  const int32_t* seg_starts_dev, int B, int total_tokens, int max_len,
                                  float* logits_out_dev, void* stream);

/* ---- late-interaction re-ranking (ColBERT-style MaxSim): one vector per token ----
 * score(query, doc) = sum over the query's tokens s of max over the doc's kept tokens t of dot(q_s, d_t).  The doc side
 * does not depend on the query: token matrices can be formed once (css_encoder_forward_tokens), kept by the caller and
 * scored later without a forward pass (css_encoder_maxsim).
 *
 * Token projection W [P, H] row-major, host fp32 (the bias-free `linear.weight` of a ColBERT checkpoint); P a multiple
 * of 32 in [32, 128].  W == NULL clears it: the token vectors are then the hidden states themselves (P = H).  Separate
 * from css_encoder_load_weights, both architectures.  May be called again.  css_encoder_token_dim: the current P. */
int css_encoder_set_token_projection(css_encoder* enc, const float* W_host /* [P,H]; NULL clears */, int P);
int css_encoder_token_dim(css_encoder* enc);
/* Packed var-len batch as css_encoder_forward.  tok_out [total_tokens, P] bf16: row t is W h_t (h_t without a
 * projection) of the final hidden state of token t, formed with fp32 accumulation from the fp32 LayerNorm output,
 * scaled to v / max(||v||, 1e-12) when normalize != 0, then rounded to bf16 once (round to nearest even).
 * seq_out [B, hidden] (may be NULL): exactly what css_encoder_forward writes.  No atomics: the same call gives the
 * same bits.  The tiny-batch graphs of css_encoder_forward are not used, created or dropped by this call.
 * _dev: device pointers (tok_out 16-byte aligned), enqueued on `stream` without a synchronise. */
int css_encoder_forward_tokens(css_encoder* enc, const int32_t* input_ids_host, const int32_t* cu_seqlens_host, int B,
                               int normalize, uint16_t* tok_out_host, float* seq_out_host);
int css_encoder_forward_tokens_dev(css_encoder* enc, const int32_t* input_ids_dev, const int32_t* cu_seqlens_dev, int B,
                                   int total_tokens, int max_len, int normalize, uint16_t* tok_out_dev, float* seq_out_dev,
                                   void* stream);
/* MaxSim over token matrices that the caller kept: no forward pass.  q_tok [sum mq, P] / d_tok [sum md, P] bf16 rows,
 * cu_q [nq + 1] / cu_d [nd + 1] their offsets (cu[0] = 0), d_keep [sum md] (may be NULL: all kept) the doc tokens that
 * take part (ColBERT's punctuation skiplist), pairs [np][2] int32 = (query, doc), scores_out [np] fp32.
 * bf16 operands, fp32 accumulation, the per-query-token maxima added in ascending s in fp32; bit reproducible.
 * P is a multiple of 32 in [32, 128], or 384, or 768 (any encoder handle serves any such P).  Every query has 1..64
 * tokens, every doc at least one kept token.  Pairs may repeat, come in any order and leave queries or docs unused;
 * np == 0 is allowed.  The host form checks all of that before anything is enqueued and names the bad query, doc or
 * pair.  _dev: device pointers (token rows 16-byte aligned), enqueued on `stream` without a synchronise; indices are
 * clamped into range, a query's tokens beyond 64 are ignored, and a doc with no kept token scores 0.
 * With few pairs a doc is spread over several blocks, whose partial maxima live in a buffer of the encoder's that only
 * grows; growing frees the old one, so work that an earlier _dev call enqueued on another stream must have finished
 * (as for the activations of css_encoder_forward_dev).  The result does not depend on the spread, bit for bit. */
int css_encoder_maxsim(css_encoder* enc, const uint16_t* q_tok_host, const int32_t* cu_q_host, int nq,
                       const uint16_t* d_tok_host, const int32_t* cu_d_host, int nd, const uint8_t* d_keep_host,
                       const int32_t* pairs_host, int np, int P, float* scores_out_host);
int css_encoder_maxsim_dev(css_encoder* enc, const uint16_t* q_tok_dev, const int32_t* cu_q_dev, int nq,
                           const uint16_t* d_tok_dev, const int32_t* cu_d_dev, int nd, const uint8_t* d_keep_dev,
                           const int32_t* pairs_dev, int np, int P, float* scores_out_dev, void* stream);
/* css_encoder_forward_tokens with normalize = 1 over the batch, then css_encoder_maxsim with the batch's sequences as
 * the docs (cu_d = cu_seqlens, nd = B; q_tok has the encoder's P columns), in one host call: nothing per token leaves
 * the device unless tok_out [total_tokens, P] is given.  Returns the bits that the two calls return. */
int css_encoder_forward_maxsim(css_encoder* enc, const int32_t* input_ids_host, const int32_t* cu_seqlens_host, int B,
                               const uint16_t* q_tok_host, const int32_t* cu_q_host, int nq, const uint8_t* d_keep_host,
                               const int32_t* pairs_host, int np, float* scores_out_host, uint16_t* tok_out_host);
int css_encoder_forward_maxsim_dev(css_encoder* enc, const int32_t* input_ids_dev, const int32_t* cu_seqlens_dev, int B,
                                   int total_tokens, int max_len, const uint16_t* q_tok_dev, const int32_t* cu_q_dev, int nq,
                                   const uint8_t* d_keep_dev, const int32_t* pairs_dev, int np, float* scores_out_dev,
                                   uint16_t* tok_out_dev, void* stream);

/* ---- learned sparse encoding (SPLADE-style): masked-LM head and a maximum over each sequence's tokens ----
 * For the final hidden state h_t of token t (the output of the last LayerNorm), with V = cfg.vocab:
 *   u_t    = gelu(Wd h_t + bd)                          erf GELU, Wd [H, H]
 *   g_t    = LayerNorm(u_t; gamma, beta, cfg.ln_eps)
 *   z[b,v] = max over the tokens t of sequence b of relu(dot(E_v, g_t) + c_v)        E [V, H], c [V]
 *   w[b,v] = (float) log1p((double) z[b,v])
 * log1p o relu is monotone, so this is SPLADE's max_t log(1 + relu(logit)) with one log1p per kept entry.  Every token
 * of the packed sequence takes part ([CLS] and [SEP] included).  z >= 0 is kept as a bit pattern in a zero-filled
 * [B, V] table under an unsigned integer atomic maximum: order-free, so the same call gives the same bits on every
 * run.  The [total_tokens, V] logits never exist in memory.  log1p is evaluated in fp64 and rounded to fp32 once, on
 * the returned entries only.
 * bf16 compute mode: g_t is rounded to bf16 once (nearest even), E is held as a bf16 copy, the products run on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation and c_v is added in fp32 after the accumulation.  The transform is
 * the fp32 GEMM over the fp32 hidden states on the unfolded paths; on the LayerNorm-folded path (hidden 768, >= 1024
 * tokens, which never materialises the fp32 hidden states) h_t and u_t are bf16 rows and the GEMM is the bf16 one.
 * fp32 compute mode (verification): fp32 throughout, products on v_mfma_f32_16x16x4_f32.
 *
 * css_encoder_set_mlm_head: host fp32 arguments, the `cls.predictions` tensors of a BertForMaskedLM: dense_w [H, H],
 * dense_b [H], ln_g / ln_b [H], decoder_w [V, H] and decoder_b [V].  decoder_w == NULL ties the decoder to the word
 * embeddings (CSS_ERR_STATE without weights): bf16 mode takes its bf16 copy of them as they are loaded NOW, fp32 mode
 * reads the encoder's own fp32 table in place, so there a later css_encoder_load_weights changes the decoder with it.
 * In either mode call this again after loading other weights.  BERT only (an MPNet encoder is CSS_ERR_INVALID).  May be
 * called again; a refused call (bad argument, wrong state, failed allocation) leaves the current head in place; a copy
 * that fails after that leaves the encoder without a head. */
int css_encoder_set_mlm_head(css_encoder* enc, const float* dense_w_host, const float* dense_b_host, const float* ln_g_host,
                             const float* ln_b_host, const float* decoder_w_host /* NULL: tied */,
                             const float* decoder_b_host);
/* The vocabulary maximum alone, no forward pass: rows [total_tokens, H] fp32 are taken as g (bf16 mode: rounded to bf16
 * on the device, then the bf16 kernel; fp32 mode: the fp32 kernel), cu_seqlens [B + 1] with cu[0] = 0 and every length
 * >= 1 (any length: max_seq_len does not apply), zmax_out [B, V] fp32 = z.  The host form checks the offsets before
 * anything is enqueued and names the bad sequence.  An MPNet encoder is CSS_ERR_INVALID, an encoder without a head
 * CSS_ERR_STATE.  _dev: device pointers, enqueued on `stream` without a synchronise; a sequence number is clamped into
 * [0, B).  In bf16 mode the rounded rows live in a buffer of the encoder's that only grows; growing frees the old one,
 * so work that an earlier _dev call enqueued on another stream must have finished (as for the activations of
 * css_encoder_forward_dev). */
int css_encoder_vocab_max(css_encoder* enc, const float* rows_host, const int32_t* cu_seqlens_host, int B,
                          float* zmax_out_host);
int css_encoder_vocab_max_dev(css_encoder* enc, const float* rows_dev, const int32_t* cu_seqlens_dev, int B, int total_tokens,
                              float* zmax_out_dev, void* stream);
/* Packed var-len batch as css_encoder_forward, then the head, the vocabulary maximum and the top-m per sequence:
 * terms_out [B, m] int32 the m largest z > 0, best first, ties to the lower term id, padded with -1; weights_out [B, m]
 * fp32 = w of those terms, padded with 0; nnz_out [B] the number of z > 0 before the cut; 1 <= m <= 512.  The
 * selection is on z and exact.  dense_out [B, V] fp32 (may be NULL) is z; rows_out [total_tokens, H] fp32 (may be
 * NULL) is g before the bf16 rounding.  The tiny-batch graphs of css_encoder_forward are not used, created or dropped
 * by this call.  Errors as css_encoder_forward, checked before anything is enqueued; an MPNet encoder is
 * CSS_ERR_INVALID, an encoder without a head CSS_ERR_STATE.  _dev: device pointers, enqueued on `stream` without a
 * synchronise; with dense_out NULL the maxima stay in a buffer of the encoder's that only grows (growth caveat as
 * above). */
int css_encoder_forward_sparse(css_encoder* enc, const int32_t* input_ids_host, const int32_t* cu_seqlens_host, int B, int m,
                               int32_t* terms_out_host, float* weights_out_host, int32_t* nnz_out_host,
                               float* dense_out_host, float* rows_out_host);
int css_encoder_forward_sparse_dev(css_encoder* enc, const int32_t* input_ids_dev, const int32_t* cu_seqlens_dev, int B,
                                   int total_tokens, int max_len, int m, int32_t* terms_out_dev, float* weights_out_dev,
                                   int32_t* nnz_out_dev, float* dense_out_dev, float* rows_out_dev, void* stream);

/* bf16 attention computes softmax rows as exp2(score) / sum WITHOUT a running maximum while every row sum of a
 * block stays in (1 / range, range) and repeats the block with the running-maximum (online) softmax otherwise --
 * same result, the guard only protects the fp32 range.  Default 2^100 (|logit| < 69); range = 0 always takes the
 * running-maximum pass (verification). */
int css_encoder_set_attention_range(css_encoder* enc, float range);

/* Test/diagnostic hook: copy an activation buffer of the LAST forward back to the
 * host as fp32 ("x32" [T,H] final hidden states, "qkv" [T,3H], "ctx" [T,H],
 * "ffn" [T,F], "pre32" [T,H]; with num_layers = 1 these are the layer-0 probes).
 * bf16 batches of >= 1024 tokens run with LayerNorm folded into the GEMM epilogues and
 * never materialise "x32" / "pre32" as such: "x32" is then an error, "pre32" / "ctx" / "ffn"
 * hold that path's buffers. */
int css_encoder_debug_read(css_encoder* enc, const char* what, float* out_host, int64_t numel);

/* Host-only helper (no device needed): bucket of a relative position
 * rel = key - query, as transformers' MPNetEncoder.relative_position_bucket
 * (the encoder builds its per-head Toeplitz bias table from it). */
int css_mpnet_rel_bucket(int rel, int num_buckets, int max_distance);

/* ---- WordPiece front end of encode() (host code; the tokenizer half of
 * SentenceTransformer.encode, src/embeddings.py:184-188, :216-222) ----
 * vocab.txt in HF layout (one piece per line, id = line number).  encode_batch:
 * `bytes` holds the n UTF-8 texts back to back, text i = [offsets[i], offsets[i+1]);
 * ids_out is [n, max_len] (padded with <pad>), lens_out[i] the token count incl.
 * <s> and </s>, or -1 for a text the tables cannot express (invalid UTF-8, a capital
 * sigma, non-ASCII text with lower-casing off), which the caller tokenises with the
 * Python implementation of the same pipeline.  nthreads <= 0: all cores. */
typedef struct css_tokenizer css_tokenizer;
int css_tokenizer_create(const char* vocab_path, int lowercase, css_tokenizer** out);
int css_tokenizer_free(css_tokenizer* t);
int css_tokenizer_vocab_size(const css_tokenizer* t, int* n);
int css_tokenizer_encode_batch(const css_tokenizer* t, const char* bytes, const int64_t* offsets,
                               int64_t n, int max_len, int32_t* ids_out, int32_t* lens_out,
                               int nthreads);

/* ---- in-library kernel timing (HIP events on the launch stream) ---- */
/* When enabled, each launch of a named dominant kernel is bracketed by HIP
 * events on the stream it is launched on; css_prof_read drains and sums them. */
int css_prof_enable(int on);
int css_prof_reset(void);
int css_prof_read(const char* kernel, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* CSS_HIP_H */
