/* ds2i_hip.h -- C ABI of libds2i_hip.so: the MI355X-native batched query path for ds2i indexes.
 *
 * ds2i has no FFI; its extension points are two C++ template concepts:
 *   Index concept     size(), num_docs(), operator[](term) -> document_enumerator
 *                     (reference block_freq_index.hpp:72-94, block_posting_list.hpp:84-186)
 *   Query-op concept  uint64_t operator()(Index const&, term_id_vec) [+ topk()]
 *                     (reference queries.hpp:35-591, driven by queries.cpp:13-62)
 * This header is what a binding for those two concepts would call. The index image and the
 * wand image are the reference's own on-disk files, unchanged (block_freq_index.hpp:124-134,
 * wand_data.hpp:71-78). Everything is plain C: no exceptions cross the boundary; every
 * function returns 0 on success or a negative DS2I_E* code, ds2i_hip_last_error() explains.
 * A handle is bound to one device and is not re-entrant; distinct handles may be used
 * concurrently from distinct host threads (index immutable, like profile_queries.cpp:25-37).
 */
#ifndef DS2I_HIP_H
#define DS2I_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* index kinds == reference index_types.hpp:18-39 */
enum ds2i_hip_index_kind {
    DS2I_BLOCK_OPTPFOR = 0,
    DS2I_BLOCK_VARINT = 1,
    DS2I_BLOCK_INTERPOLATIVE = 2,
    DS2I_BLOCK_QMX = 3,
    DS2I_BLOCK_MIXED = 4,
    DS2I_OPT = 5,     /* opt_index: freq_index<partitioned_sequence<>, positive_sequence<partitioned_sequence<strict_sequence>>>
                         (index_types.hpp:29-32) */
    DS2I_EF = 6,      /* ef_index: freq_index<compact_elias_fano, positive_sequence<strict_elias_fano>> (index_types.hpp:18-19) */
    DS2I_SINGLE = 7,  /* single_index: freq_index<indexed_sequence, positive_sequence<>> (index_types.hpp:21-22) */
    DS2I_UNIFORM = 8  /* uniform_index: freq_index<uniform_partitioned_sequence<>,
                         positive_sequence<uniform_partitioned_sequence<strict_sequence>>> (index_types.hpp:24-27) */
};

/* query operators == the strings queries.cpp:104-117 dispatches on (+ ranked_or, queries.hpp:404) */
enum ds2i_hip_op {
    DS2I_OP_AND = 0,        /* and_query<false>   queries.hpp:35-86   */
    DS2I_OP_AND_FREQ = 1,   /* and_query<true>                        */
    DS2I_OP_OR = 2,         /* or_query<false>    queries.hpp:88-131  */
    DS2I_OP_OR_FREQ = 3,    /* or_query<true>                         */
    DS2I_OP_RANKED_AND = 4, /* ranked_and_query   queries.hpp:322-401 */
    DS2I_OP_WAND = 5,       /* wand_query         queries.hpp:200-319 */
    DS2I_OP_MAXSCORE = 6,   /* maxscore_query     queries.hpp:478-591 */
    DS2I_OP_RANKED_OR = 7,  /* ranked_or_query    queries.hpp:404-476 */
    /* OR this flag into any operator to run the reference's
       one-document-per-step traversal on the GPU instead of the block-synchronous kernel (same results; used to
       cross-check and to count the reference traversal's algorithmic bytes on the device). */
    DS2I_OP_REFERENCE_ORDER = 0x100,
    /* OR this flag into the operator of ds2i_hip_query_batch / ds2i_hip_pipeline_submit to run the kernels compiled
       without the statistics counters even though a stats struct is passed (it then carries kernel_ms only). */
    DS2I_OP_NO_COUNTERS = 0x200,
    /* OR this flag into a ranked operator (ranked_and / wand / maxscore / ranked_or) of ds2i_hip_batch_prepare,
       ds2i_hip_pipeline_submit or ds2i_hip_query_batch_docs to get the doc-id of every top-k score as well
       (ds2i_hip_batch_fetch_topk_docs / ds2i_hip_pipeline_wait_docs). Each row is ordered by score descending, equal
       scores by doc-id ascending, and holds the k largest (score, -doc-id) pairs: on a tie at the k-th place the smaller
       doc-ids are returned. Entries past the row's length are 0xFFFFFFFF. Scores, lengths and counts are the same bits as
       without the flag. With and / and_freq / or / or_freq, or with ds2i_hip_query_batch: DS2I_EINVAL. A docs batch
       reports no counters, as with DS2I_OP_NO_COUNTERS (stats carry kernel_ms only; its kernels are the uninstrumented
       instantiations wherever a kernel has one), and ds2i_hip_batch_enable_block_profile refuses it (DS2I_EINVAL). */
    DS2I_OP_TOPK_DOCS = 0x400
};

enum ds2i_hip_error {
    DS2I_OK = 0,
    DS2I_EINVAL = -1,   /* bad argument (null pointer, unknown kind/op, k out of range) */
    DS2I_EFORMAT = -2,  /* index / wand image failed validation */
    DS2I_ETERM = -3,    /* term id >= index size (UB + assert in the reference, block_freq_index.hpp:87) */
    DS2I_EDEVICE = -4,  /* HIP runtime error or no usable device */
    DS2I_ENOWAND = -5,  /* ranked operator without wand data (queries.cpp:108-116 logs "Unsupported") */
    DS2I_ETOOLONG = -6, /* query has more than DS2I_HIP_MAX_TERMS_LONG distinct terms */
    DS2I_ENOMEM = -7,
    DS2I_EBUSY = -8     /* pipeline: every slot is in flight -- collect the oldest ticket first */
};

#define DS2I_HIP_MAX_TERMS 16        /* distinct terms per query held in LDS by one wavefront (the fast kernels) */
#define DS2I_HIP_MAX_TERMS_LONG 1024 /* beyond 16 distinct terms a query runs the one-document-per-step traversal with
                                        its enumerator state in global memory (the reference has no limit, queries.hpp:35-86) */
#define DS2I_HIP_MAX_K 64            /* top-k kept one score per lane (the fast kernels) */
#define DS2I_HIP_MAX_K_LONG 1024     /* beyond 64 the same stream kernels run with 4 (k <= 256) or 16 scores per lane; only a
                                        batch that also holds a query of more than 16 terms, or a natively queried block_mixed
                                        image, falls to the one-document-per-step kernel (the reference's topk_queue has no
                                        limit, queries.hpp:152-197) */

typedef struct ds2i_hip_index ds2i_hip_index;
typedef struct ds2i_hip_batch ds2i_hip_batch;

/* Device-side counters of one batch run; the byte pricing is SURVEY.md §8(d)'s A_skip. */
typedef struct ds2i_hip_stats {
    double kernel_ms;             /* device-side WINDOW of the last run (hipEvents): from the batch's first clear to the
                                     completion of its last kernel. In a pipeline the window also holds whatever other
                                     batches ran on the GPU meanwhile; for wand / maxscore / ranked_or the ranked_and seed
                                     pass is enqueued ahead of the window and may start before it. rocprofv3's per-kernel
                                     durations are the exact figures. */
    uint64_t docs_blocks_decoded; /* block_profiler counter [2b]   (block_posting_list.hpp:316-318) */
    uint64_t freqs_blocks_decoded;/* block_profiler counter [2b+1] (block_posting_list.hpp:328-330) */
    uint64_t block_max_examined;
    uint64_t algorithmic_bytes;
    uint64_t postings_scored;
    uint64_t rounds;              /* block-synchronous rounds (conjunctive kernel) */
} ds2i_hip_stats;

int ds2i_hip_device_count(void);
/* Tuning knobs without the environment: name = one of the twenty documented DS2I_*
 * variables, value = what the variable would hold (NULL = unset). Process-wide like the variables themselves; every
 * ds2i_hip_index_open re-reads them, and they hold for that index and the batches planned until the next upload. Unknown names
 * fail with DS2I_EINVAL. */
int ds2i_hip_set_option(const char* name, const char* value);
const char* ds2i_hip_last_error(void);

/* Copies the index (and optional wand data) to the device's HBM. The images are not referenced
 * after the call returns. Replaces succinct::mapper::map of queries.cpp:76-77,90-95.
 * block_mixed and the freq_index layouts (opt / ef / single / uniform) are decoded once on the device and queried as
 * block_optpfor (same postings, same answers; ds2i_hip_index_info::transcoded_from says so); DS2I_MIXED_NATIVE=1 /
 * DS2I_PEF_NATIVE=1 in the environment (or ds2i_hip_set_option) keep the image and run its own kernels. */
int ds2i_hip_index_open(int device, int index_kind, const void* index_image, size_t index_bytes,
                        const void* wand_image, size_t wand_bytes, ds2i_hip_index** out);
void ds2i_hip_index_close(ds2i_hip_index* idx);

/* Index concept: size() = number of posting lists, num_docs() (block_freq_index.hpp:72-80) */
uint64_t ds2i_hip_index_size(const ds2i_hip_index* idx);
uint64_t ds2i_hip_index_num_docs(const ds2i_hip_index* idx);
uint64_t ds2i_hip_index_device_bytes(const ds2i_hip_index* idx);
/* Collection-wide BM25 statistics on an open index, for an index that holds a shard of a collection: every batch planned afterwards
 * (one-shot, prepared and pipelined alike) weighs a query term by bm25::query_term_weight(qtf, df[term], num_docs) instead of the
 * list's own length and the index's own number of documents. Nothing else changes: list order, work units, routes and kernel choice
 * keep using the shard's own list lengths, and the bounds that are products of the query weight follow from it as before (wand /
 * maxscore / ranked_or as streams drive a query by its lists in the order of those bounds and give no units to the lists whose bounds
 * lie below the query's static floor, as they always did: there the units follow from the query weight too). df has
 * ndf == ds2i_hip_index_size(idx) entries and is copied. num_docs == 0 && df == NULL clears the statistics. Checks, in this order, all
 * DS2I_EINVAL, nothing changed on an error: null index; ndf != ds2i_hip_index_size(idx) (or df == NULL with num_docs != 0); num_docs <
 * ds2i_hip_index_num_docs(idx); the first term whose df[t] is below its list length or above num_docs, named. Batches already prepared
 * keep their weights. The call must NOT run concurrently with planning on the same index (prepare, submit or a one-shot query on
 * another thread): the handle is not re-entrant. */
int ds2i_hip_index_set_collection_stats(ds2i_hip_index* idx, uint64_t num_docs, const uint32_t* df, uint64_t ndf);
/* What the upload put into HBM beside the index image. The pruning tables are accelerators: an upload that cannot
 * afford them (or was told not to build them) still succeeds and the query kernels take their slower table-free paths,
 * so a caller that cares checks has_range_tables here (the library also says so once on stderr). With
 * DS2I_RMW_REQUIRE=1 in the environment such an upload fails with DS2I_ENOMEM instead. */
typedef struct ds2i_hip_index_info {
    uint64_t index_bytes;        /* the posting lists (block indexes) / chunk directory + bit vectors (freq_index layouts) */
    uint64_t skip_table_bytes;   /* interleaved {block_max, end offset} rows (block indexes) */
    uint64_t block_weight_bytes; /* bmw[]: one float per block / chunk */
    uint64_t range_table_bytes;  /* doc-id-range tables, their two coarser levels, membership bit tables, dense bitmaps */
    uint64_t norm_len_bytes;
    uint64_t total_blocks;
    uint64_t total_postings;
    int has_block_weights;
    int has_range_tables;
    int has_bitmaps;
    int has_membership_hints;    /* one more byte per level-1 range-table entry (block_optpfor indexes): see ds2i_hip_list_range_table */
    int range_table_entries_per_posting; /* DS2I_RMW_G in effect */
    uint64_t side_table_bytes;   /* block_optpfor: exception side slots (256 B per block: the OptPFor exceptions of a block as position
                                  * masks + values, so that a decode never parses the Simple16 streams), their overflow area, and the
                                  * lists' partial last blocks in plain form; 0 = not built (DS2I_NO_XSLOTS, other index kinds, no room) */
    int has_side_tables;
    int transcoded_from;         /* the DS2I_* kind of the image the caller handed over when the upload transcoded it to block_optpfor
                                  * (block_mixed, opt / ef / single / uniform by default: DS2I_MIXED_NATIVE / DS2I_PEF_NATIVE), else -1 */
    uint64_t table_budget_bytes; /* DS2I_TABLE_BUDGET in effect at the upload (bytes; 0 = none): the upload built the first of
                                  * {tables at 4 / 2 / 1 entries per posting} x {hints} x {side slots} whose resident bytes fit --
                                  * range_table_entries_per_posting, has_membership_hints, has_side_tables say which */
} ds2i_hip_index_info;
int ds2i_hip_index_get_info(const ds2i_hip_index* idx, ds2i_hip_index_info* out);
/* document_enumerator::size() of index[term] (block_posting_list.hpp:178-181) */
int ds2i_hip_list_size(const ds2i_hip_index* idx, uint32_t term, uint64_t* n);
/* index[term] followed by a full enumeration docid()/freq()/next(): decodes every block of the
 * list on the GPU. docs/freqs hold `capacity` entries; *n receives the list length. */
int ds2i_hip_decode_list(ds2i_hip_index* idx, uint32_t term, uint32_t* docs, uint32_t* freqs, uint64_t capacity,
                         uint64_t* n);

/* One-shot batched query operator: for each query q (terms[query_offsets[q] .. query_offsets[q+1]))
 *   out_count[q]    the operator's return value (matches for and/or, top-k size for ranked ops)
 *   out_topk        nq*k floats, each query's scores descending, padded with -inf. Ranked operators only:
 *                   and / or produce no top-k, ignore k and never touch out_topk (may be NULL)
 *   out_topk_len    nq (may be NULL)
 * Host terms -> HBM, kernels, results -> host. The batch slot (pinned staging, device blocks, events) is cached in
 * the index handle: repeated calls allocate nothing. stats may be NULL; when given, the instrumented kernels run
 * (counters filled) unless DS2I_OP_NO_COUNTERS is set. A query may have any number of distinct terms up to
 * DS2I_HIP_MAX_TERMS_LONG (the reference has no limit); beyond DS2I_HIP_MAX_TERMS it takes the slower long path. */
int ds2i_hip_query_batch(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms,
                         const uint32_t* query_offsets, uint32_t nq, uint64_t* out_count, float* out_topk,
                         uint32_t* out_topk_len, ds2i_hip_stats* stats);
/* ds2i_hip_query_batch with DS2I_OP_TOPK_DOCS in op (required): out_topk_docs has nq*k entries */
int ds2i_hip_query_batch_docs(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms,
                              const uint32_t* query_offsets, uint32_t nq, uint64_t* out_count, float* out_topk,
                              uint32_t* out_topk_docs, uint32_t* out_topk_len, ds2i_hip_stats* stats);

/* Split form: prepare() does query normalisation (query_freqs / remove_duplicate_terms,
 * queries.hpp:29-33,136-150), BM25 query weights, list-length ordering and uploads everything;
 * run() only launches kernels on data already resident in HBM (this is what bench.py times);
 * fetch() copies results back. want_matches != 0 additionally collects the doc-id lists of `and`. */
int ds2i_hip_batch_prepare(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms,
                           const uint32_t* query_offsets, uint32_t nq, int want_matches, ds2i_hip_batch** out);
int ds2i_hip_batch_run(ds2i_hip_batch* b, ds2i_hip_stats* stats);
/* Statistics are an instrumentation option like the reference's block_profiler (`template <bool Profile>`,
 * block_posting_list.hpp:316-318): with on = 0 the conjunctive operators on block_optpfor / opt run kernels compiled
 * without the counters (faster; ds2i_hip_stats then carries kernel_ms only and the per-class counters keep the values
 * of the last instrumented run). Default: on. */
int ds2i_hip_batch_set_instrumented(ds2i_hip_batch* b, int on);

/* Block access profile of a batch on a block index (the GPU-side profile_queries.cpp, reference
 * profile_queries.cpp:21-95): after enable, every instrumented run adds, for each 128-posting block of the index,
 * the number of docs-part and freqs-part decodes. counts receives 2 x total_blocks values, blocks numbered list by
 * list in index order (block b of list t at 2 * (sum_{u<t} ceil(n_u/128) + b)). Pass counts = NULL to query
 * total_blocks only. Input of the block_mixed optimiser (ds2i_hybrid_*, ds2i_build.h). */
int ds2i_hip_batch_enable_block_profile(ds2i_hip_batch* b);
int ds2i_hip_batch_block_profile(ds2i_hip_batch* b, uint32_t* counts, uint64_t capacity, uint64_t* total_blocks);
/* per kernel class of the last run (class 0: <=2 distinct terms, 1: 3..4, 2: 5..8, 3: 9..16 -- four
 * template instantiations with different LDS footprints -- 4: more than 16; launched concurrently on their own streams) */
int ds2i_hip_batch_class_stats(ds2i_hip_batch* b, int cls, ds2i_hip_stats* out, uint32_t* nqueries);
/* A class may run more than one kernel: ranked_and on a block_optpfor index launches the pipelined stream kernel once per
 * exact list count (2, 3, 4 terms) and the class kernel for what is left (one-term queries), back to back on the class
 * stream. Per launch group of class cls in the last run: the hipEvent duration on that stream, the list slots the kernel
 * was launched with, its units (= workgroups) and queries. out may be NULL to ask for *ngroups only. */
typedef struct ds2i_hip_group_stats {
    double kernel_ms;
    uint32_t lists, units, queries;
    int pipelined_stream; /* 1: k_ranked_stream<lists> (ranked_stream.hip); 0: the class kernel */
} ds2i_hip_group_stats;
int ds2i_hip_batch_class_groups(ds2i_hip_batch* b, int cls, ds2i_hip_group_stats* out, uint32_t capacity, uint32_t* ngroups);
/* diagnostic build only (-DDS2I_PHASE_TIMING): per-phase shader-cycle sums {total, docs decode, freqs
 * decode, block search, membership, scoring, top-k} of class cls; zeros otherwise */
int ds2i_hip_batch_phase_cycles(ds2i_hip_batch* b, int cls, uint64_t* out, int n);
int ds2i_hip_batch_fetch(ds2i_hip_batch* b, uint64_t* out_count, float* out_topk, uint32_t* out_topk_len,
                         uint64_t* out_freq_sum);
/* doc-id lists of `and` (want_matches): match_offsets has nq+1 entries; matches has match_offsets[nq] */
int ds2i_hip_batch_match_total(ds2i_hip_batch* b, uint64_t* total);
int ds2i_hip_batch_fetch_matches(ds2i_hip_batch* b, uint64_t* match_offsets, uint32_t* matches);
/* doc-ids of the top-k (DS2I_OP_TOPK_DOCS): nq*k entries, same layout as out_topk; DS2I_EINVAL on a batch prepared without the flag */
int ds2i_hip_batch_fetch_topk_docs(ds2i_hip_batch* b, uint32_t* out_docs);
void ds2i_hip_batch_free(ds2i_hip_batch* b);

/* Pipelined form -- the serving loop. A pipeline owns `depth` reusable batch slots. submit() does the host half of
 * the operator (query normalisation, BM25 query weights, work-unit planning: queries.hpp:29-33,136-150,357-360),
 * then enqueues ONE async H2D copy, the kernels and ONE async D2H copy of the results and returns without waiting
 * for the device: the host plans batch i+1 while the kernels of batch i run, and the kernels of consecutive batches
 * overlap on the device. wait() blocks until the ticket's batch is complete and copies its results out (same
 * meaning as ds2i_hip_query_batch). Tickets must be collected before their slot comes round again (submit() returns
 * DS2I_EBUSY otherwise). This is the loop queries.cpp:25-35 becomes: every query is timed fresh, nothing is
 * pre-staged on the device. */
typedef struct ds2i_hip_pipeline ds2i_hip_pipeline;
int ds2i_hip_pipeline_create(ds2i_hip_index* idx, uint32_t depth, ds2i_hip_pipeline** out);
int ds2i_hip_pipeline_submit(ds2i_hip_pipeline* p, int op, uint32_t k, const uint32_t* terms,
                             const uint32_t* query_offsets, uint32_t nq, uint64_t* ticket);
int ds2i_hip_pipeline_wait(ds2i_hip_pipeline* p, uint64_t ticket, uint64_t* out_count, float* out_topk,
                           uint32_t* out_topk_len, ds2i_hip_stats* stats);
/* wait() with the doc-ids of a ticket submitted with DS2I_OP_TOPK_DOCS (out_topk_docs: nq*k entries, or NULL). A ticket
 * submitted without the flag and a non-NULL out_topk_docs: DS2I_EINVAL, and the ticket stays uncollected. Plain wait()
 * on a docs ticket returns its scores and drops the ids. */
int ds2i_hip_pipeline_wait_docs(ds2i_hip_pipeline* p, uint64_t ticket, uint64_t* out_count, float* out_topk,
                                uint32_t* out_topk_docs, uint32_t* out_topk_len, ds2i_hip_stats* stats);
/* like ds2i_hip_batch_class_stats, for the ticket collected last */
int ds2i_hip_pipeline_class_stats(ds2i_hip_pipeline* p, int cls, ds2i_hip_stats* out, uint32_t* nqueries);
int ds2i_hip_pipeline_class_groups(ds2i_hip_pipeline* p, int cls, ds2i_hip_group_stats* out, uint32_t capacity, uint32_t* ngroups);
/* default off: pipelines run the kernels compiled without counters */
int ds2i_hip_pipeline_set_instrumented(ds2i_hip_pipeline* p, int on);
void ds2i_hip_pipeline_destroy(ds2i_hip_pipeline* p);

/* GPU index encoder (build side): block_posting_list::write (block_posting_list.hpp:13-53) with
 * optpfor_block::encode + ds2i's findBestB (block_codecs.hpp:156-208) as HIP kernels, one wavefront per 128-posting
 * block. Input: nlists posting lists in CSR form (list t = docs / freqs [list_offsets[t], list_offsets[t+1])), sorted
 * doc-ids < num_docs, freqs >= 1. Output: the frozen block_freq_index image of that kind (ds2i_blob_* of
 * ds2i_build.h release it), byte-identical to the host builder's (ds2i_builder_*). index_kind is DS2I_BLOCK_OPTPFOR,
 * DS2I_BLOCK_VARINT (every full block VarInt-G8IU) or DS2I_BLOCK_INTERPOLATIVE; DS2I_BLOCK_QMX has no GPU encoder and
 * DS2I_BLOCK_MIXED images come from ds2i_hip_hybrid_freeze below: both are DS2I_EINVAL here. device_ms (may be NULL)
 * receives the hipEvent time of the kernels the call ran.
 * The Elias-Fano layouts -- DS2I_OPT, DS2I_EF, DS2I_SINGLE, DS2I_UNIFORM -- are encoded too: the image is the one
 * ds2i_builder_create(kind, num_docs) / ds2i_builder_add_posting_list x nlists / ds2i_builder_freeze return, byte for
 * byte, with the default global_parameters (sampling 9 / 8 / 9 / 8, log_partition_size 7). Every size of these layouts
 * is an integer in closed form of (universe, n), so the host plans -- type, length and final bit offset of every base
 * sequence, the headers -- and, for DS2I_OPT, takes the partition end points from the device planner
 * (ds2i_hip_encode_index_with below chooses between it and optimal_partition on at most 16 host threads); HIP kernels form the prefix sums of the freqs and write every base sequence (Elias-Fano, ranked
 * bitvector, their sampled arrays) into the two bit vectors, one thread per posting. For these kinds the input is
 * checked on the host before anything is staged: an empty list ("List must be nonempty"), doc-ids not strictly
 * increasing or >= num_docs, and a zero freq are DS2I_EINVAL; no output is written on an error. */
typedef struct ds2i_blob ds2i_blob;
int ds2i_hip_encode_index(int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                          const uint32_t* docs, const uint32_t* freqs, ds2i_blob** image, double* device_ms);
/* Diagnostic: the host seconds of this thread's last ds2i_hip_encode_index / ds2i_hip_build_collection of an Elias-Fano kind:
 * seconds[0] planning on the host (DS2I_OPT: the partition DP when the host plans it; headers and jobs either way),
 * seconds[1] download, headers and freeze. */
void ds2i_hip_encode_host_seconds(double seconds[2]);

/* ds2i_hip_encode_index with a choice of who plans the partitions of DS2I_OPT (the (1+eps)-approximate shortest path of
 * optimal_partition, per list and side): DS2I_ENCODE_PLAN_HOST -- list-parallel on at most 16 host threads;
 * DS2I_ENCODE_PLAN_DEVICE -- HIP kernels, one wavefront per list and side over the staged postings (cost classes are lanes; the
 * classes' budgets, the DP's only floating point, come from the host). flags == 0 takes the default, which is what
 * ds2i_hip_encode_index, ds2i_hip_build_collection and ds2i_hip_convert_index take: the device planner. Both bits set is
 * DS2I_EINVAL. The end points are the same either way, so the image is the same, byte for byte. Kinds without a DP ignore
 * the two bits. Everything else is ds2i_hip_encode_index. */
enum { DS2I_ENCODE_PLAN_HOST = 1u, DS2I_ENCODE_PLAN_DEVICE = 2u };
int ds2i_hip_encode_index_with(int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                               const uint32_t* docs, const uint32_t* freqs, uint32_t flags, ds2i_blob** image, double* device_ms);
/* Diagnostic: the hipEvent milliseconds of the partition kernels in this thread's last encode call (ds2i_hip_encode_index[_with],
 * ds2i_hip_build_collection, ds2i_hip_convert_index); 0.0 when the host planned or the kind has no DP. */
void ds2i_hip_encode_plan_ms(double* ms);
/* The device planner alone: the partition end points DS2I_OPT takes for every list of a collection (CSR form and input checks of
 * ds2i_hip_encode_index's Elias-Fano kinds, made before anything is staged). Per side -- docs: the doc-ids over num_docs; freqs:
 * the strict prefix sums of the freqs over occurrences + 1 -- *_ends receives the exclusive end index of every partition of every
 * list back to back (u32; a list's last one is its length) and *_offs nlists + 1 u64 offsets into it. The same four blobs as
 * ds2i_opt_partition (ds2i_build.h), the host DP, element for element. scratch_bytes: the DP scratch (12 bytes per posting and
 * side) one group of consecutive lists may take, 0 = the default (2 GiB); a group holds at least one list. device_ms (may be
 * NULL): the hipEvent time of the kernels. No output is written on an error. */
int ds2i_hip_opt_partition(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                           const uint32_t* freqs, uint64_t scratch_bytes, ds2i_blob** docs_ends, ds2i_blob** docs_offs,
                           ds2i_blob** freqs_ends, ds2i_blob** freqs_offs, double* device_ms);

/* wand_data on the GPU (build side; create_wand_data.cpp:8-29, wand_data.hpp:20-52): the image ds2i_wand_create(doc_sizes,
 * num_docs) / ds2i_wand_add_list x nlists / ds2i_wand_freeze of ds2i_build.h return for the same input, byte for byte.
 * They live here because nothing in ds2i_build.h touches the GPU. Lists in the CSR form of ds2i_hip_encode_index;
 * doc_sizes holds num_docs (> 0) document lengths. norm_lens are computed on the host exactly as the host builder
 * computes them; max_term_weight[t] = max over list t's postings of bm25::doc_term_weight(freq, norm_len[doc]) comes from
 * a HIP kernel, one wavefront per 128-posting block, with the query kernels' own scoring function.
 * An empty list ("List must be nonempty") and a doc-id >= num_docs (checked on the host, before anything is launched)
 * are DS2I_EINVAL. device_ms (may be NULL) receives the hipEvent time of the kernel. */
int ds2i_hip_build_wand(int device, const uint32_t* doc_sizes, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                        const uint32_t* docs, const uint32_t* freqs, ds2i_blob** wand_image, double* device_ms);
/* Both images of a collection from ONE staging of its postings: everything ds2i_hip_index_open needs. index_image is what
 * ds2i_hip_encode_index(index_kind, ...) returns (same kinds, the Elias-Fano layouts among them, and the same input
 * checks; DS2I_BLOCK_QMX and DS2I_BLOCK_MIXED are DS2I_EINVAL), wand_image what ds2i_hip_build_wand returns. wand_image
 * may be NULL (doc_sizes may then be NULL too); on an error neither output is written. device_ms (may be NULL): the
 * hipEvent time of the encoder's kernels plus the wand kernel. */
int ds2i_hip_build_collection(int device, int index_kind, const uint32_t* doc_sizes, uint64_t num_docs, uint64_t nlists,
                              const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                              ds2i_blob** index_image, ds2i_blob** wand_image, double* device_ms);

/* The block_mixed optimiser of ds2i_build.h (ds2i_hybrid_*) with its build side on the GPU. They
 * live here because nothing in ds2i_build.h touches the GPU; the handle is the one ds2i_hybrid_create returns, filled
 * with ds2i_hybrid_add_posting_list. A builder that holds virtual lists (ds2i_synth_build_hybrid) is DS2I_EINVAL.
 * analyse: a plan kernel measures every candidate of every 128-value part (OptPFor at each usable b, VarInt-G8IU,
 * interpolative: sizes and counts, integers only); the host turns them into the same (space, time) hulls as
 * ds2i_hybrid_analyse, bit for bit, so either analysis serves either freeze, ds2i_hybrid_hull included.
 * freeze: solves the budget on the host as ds2i_hybrid_freeze does (analysing on the device first if need be) and
 * writes the chosen encodings in one kernel pass; image, rate, space, model_time and type_counts equal the host's.
 * device_ms (may be NULL) receives the hipEvent time of the kernels this call ran. */
struct ds2i_hybrid;
int ds2i_hip_hybrid_analyse(struct ds2i_hybrid* h, int device, uint64_t* min_space, uint64_t* max_space, double* device_ms);
int ds2i_hip_hybrid_freeze(struct ds2i_hybrid* h, int device, uint64_t budget_bytes, ds2i_blob** image, double* rate,
                           uint64_t* space, double* model_time, uint64_t type_counts[6], double* device_ms);

/* The synthetic collection of ds2i_build.h generated on `threads` host threads (<= 0: all) and encoded on the GPU;
 * the same two images as ds2i_synth_build(p, DS2I_BLOCK_OPTPFOR, ...), byte for byte (one staging, as
 * ds2i_hip_build_collection: the maximum term weights come from the wand kernel). wand_image, total_postings,
 * generate_s (host seconds spent generating the lists) and device_ms may be NULL. */
struct ds2i_synth_params;
int ds2i_hip_synth_encode(int device, const struct ds2i_synth_params* p, int threads, ds2i_blob** index_image,
                          ds2i_blob** wand_image, uint64_t* total_postings, double* generate_s, double* device_ms);

/* Verification of an index against the collection it was built from (the last step of the reference's
 * create_freq_index --check): every list of the index is decoded on the GPU -- ONE launch over all blocks (chunks) of all lists,
 * one wavefront per block, with the decoders the query and decode paths use -- and every doc-id and freq compared with the
 * collection, staged once in HBM in the CSR form of ds2i_hip_encode_index. Only the first difference comes back.
 * The report: `what` says what differs first, in this order: the number of documents, the number of lists, the length of a list
 * (these three on the host, before any device is touched), then the first posting in (list, position) order whose doc-id
 * differs, or whose doc-id matches and whose freq differs -- the same answer whatever the scheduling. `got` is what the index
 * holds, `expected` what the collection holds: DS2I_VERIFY_NUM_DOCS / _LISTS fill got / expected only, _LENGTH fills list and the
 * two lengths, _DOCID / _FREQ fill all four. postings_checked: the postings before the first difference (all of them when
 * what == DS2I_VERIFY_OK). device_ms (may be NULL): the hipEvent time of the kernel; 0 when no kernel ran.
 * The return code is DS2I_OK whenever the comparison ran, difference or not; errors are bad arguments (DS2I_EINVAL: a null
 * pointer, an unknown kind, list_offsets not starting at 0 or decreasing), a bad image (DS2I_EFORMAT), the device, memory.
 * The collection is staged whole beside the index: 8 bytes per posting of device memory.
 * Like the reference's check this is for images a builder wrote: an image's structure is trusted exactly as far as
 * ds2i_hip_index_open trusts it, and the decoders are not hardened against hostile payload bytes. */
enum ds2i_hip_verify_what {
    DS2I_VERIFY_OK = 0,
    DS2I_VERIFY_NUM_DOCS = 1,
    DS2I_VERIFY_LISTS = 2,
    DS2I_VERIFY_LENGTH = 3,
    DS2I_VERIFY_DOCID = 4,
    DS2I_VERIFY_FREQ = 5
};
typedef struct ds2i_hip_verify_report {
    int what;
    uint64_t list, position, got, expected;
    uint64_t postings_checked;
} ds2i_hip_verify_report;
/* The handle as queries read it: the transcoded image when the upload transcoded; block_optpfor with side tables through the
 * side-slot decoder of the stream kernels, or the general decoders under DS2I_DECODE_GENERAL (the choice ds2i_hip_decode_list makes). */
int ds2i_hip_index_verify(ds2i_hip_index* idx, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                          const uint32_t* docs, const uint32_t* freqs, ds2i_hip_verify_report* report, double* device_ms);
/* The caller's bytes with the on-disk decoders of that kind (all nine kinds): the image is parsed on the host, the structure
 * compared, and only then uploaded bare (no tables, no transcoding), verified by the same kernel and closed. */
int ds2i_hip_verify_collection(int device, int index_kind, const void* image, size_t bytes, uint64_t num_docs, uint64_t nlists,
                               const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                               ds2i_hip_verify_report* report, double* device_ms);
/* Diagnostic: the host seconds of this thread's last verification: seconds[0] the host parse of the image and the structure
 * comparison (ds2i_hip_verify_collection only), seconds[1] its bare upload (likewise), seconds[2] the staging of the postings. */
void ds2i_hip_verify_host_seconds(double seconds[3]);

/* Extraction: the postings back out of an index, and an image of one kind turned into an image of another. The decode is the
 * verification's -- ONE launch over all blocks (chunks) of the lists asked for, one wavefront per block -- with stores instead of
 * compares: the postings land in CSR form (the form of ds2i_hip_encode_index) in two device buffers of exactly the postings' size,
 * 8 bytes per posting beside the index; what does not fit is DS2I_ENOMEM (there is no chunked form). device_ms (may be NULL): the
 * hipEvent time of the kernels; 0 when none ran. An index holds neither the document sizes nor wand data: they do not come back.
 *
 * ds2i_hip_index_extract: lists [list_begin, list_end) of an open index as queries read it (the transcoded image when the upload
 * transcoded; the decoder choice of ds2i_hip_index_verify). list_offsets receives list_end - list_begin + 1 offsets, from 0;
 * *postings their last. docs == NULL and freqs == NULL is the size query: offsets and *postings only, nothing is launched (one of
 * the two NULL is DS2I_EINVAL). list_begin > list_end or list_end > size is DS2I_EINVAL; a capacity (in postings) below *postings
 * is DS2I_EINVAL with *postings set to what is needed. */
int ds2i_hip_index_extract(ds2i_hip_index* idx, uint64_t list_begin, uint64_t list_end, uint64_t* list_offsets, uint32_t* docs,
                           uint32_t* freqs, uint64_t capacity, uint64_t* postings, double* device_ms);
/* The whole collection out of the caller's bytes with the on-disk decoders of that kind (all nine kinds), in the order of
 * ds2i_hip_verify_collection: argument checks, the image parsed on the host (a bad image is ds2i_hip_index_open's DS2I_EFORMAT), only
 * then the device: a bare upload (no tables, no transcoding), the kernel, close. list_offsets: u64[*nlists + 1]; docs / freqs:
 * u32[postings]; free each with ds2i_blob_free. On an error no output is written. */
int ds2i_hip_extract_collection(int device, int index_kind, const void* image, size_t bytes, uint64_t* num_docs, uint64_t* nlists,
                                ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs, double* device_ms);
/* An image of from_kind (any of the nine) as an image of to_kind, byte-identical to what the host builder writes for the same
 * postings. to_kind: a kind ds2i_hip_encode_index writes (DS2I_BLOCK_QMX and DS2I_BLOCK_MIXED are DS2I_EINVAL, checked before the
 * image is read), with that function's input rules (the Elias-Fano layouts: doc-ids strictly increasing, freqs >= 1). Bare upload,
 * extraction into device buffers, the source image closed, then the encoder over the postings where they lie: for the block
 * codecs they never leave the device, for the Elias-Fano layouts they come down once, for the host planner. device_ms: the
 * extraction kernel plus the encoder's kernels. */
int ds2i_hip_convert_index(int device, int from_kind, const void* image, size_t bytes, int to_kind, ds2i_blob** out_image,
                           double* device_ms);
/* Diagnostic: the host seconds of this thread's last ds2i_hip_extract_collection: seconds[0] the host parse of the image,
 * seconds[1] its bare upload, seconds[2] the copy of the postings to the host. */
void ds2i_hip_extract_host_seconds(double seconds[3]);

/* Renumbering the documents on the GPU: new doc-id = doc_map[old doc-id], doc_map a permutation of [0, num_docs) (ds2i_check_doc_map,
 * ds2i_build.h, run before any device is touched). List lengths and list order do not change; within every list the postings are
 * sorted again by their new doc-ids and the freqs travel with them. The doc-ids of a list are distinct, so the result is unique: it
 * is ds2i_remap_postings' (ds2i_build.h, the host twin), element for element. A map kernel sends every doc-id through the map; the
 * sort is planned on the host from the list lengths into three classes (ds2i_hip_remap_class_bounds: W, L, T): lists of up to W
 * postings are sorted in the registers of one wavefront each, lists of up to L in the LDS of one workgroup each, and the longer ones
 * together, in tiles of T postings, by an LSD radix sort over the key bits num_docs needs, between two buffer pairs. No kernel
 * waits for another workgroup; the order between the steps is the order of the launches on one stream.
 *
 * ds2i_hip_remap_postings: a collection in (CSR form of ds2i_hip_encode_index; empty lists are allowed), the renumbered collection
 * out; out_docs / out_freqs hold list_offsets[nlists] words each and may be docs / freqs. Checks, in this order: null arguments and
 * the offsets (DS2I_EINVAL), the map (DS2I_EINVAL), the device (DS2I_EDEVICE). A doc-id >= num_docs among the postings is found by
 * the map kernel, which never reads past the map: DS2I_EFORMAT, no output written. Device memory: 16 bytes per posting, 4 per
 * document. device_ms (may be NULL): the hipEvent time of the kernels.
 *
 * ds2i_hip_remap_index: an image of from_kind (any of the nine) as the image of to_kind of the renumbered collection, byte-identical
 * to the host builder's over the host twin's lists. to_kind as ds2i_hip_convert_index takes it (DS2I_BLOCK_QMX and DS2I_BLOCK_MIXED
 * are DS2I_EINVAL, same message). Checks, in this order: null arguments, the kinds, the host parse of the image (DS2I_EFORMAT),
 * map_len == the image's number of documents, the map, the device. Then ds2i_hip_convert_index's steps with one more: bare upload,
 * extraction, the source image closed, map and sort, the sort's second buffer pair freed, the encoder over the postings where
 * they lie. The postings never cross the bus for a block codec target. Peak device memory: the image + 8 bytes per posting while
 * extracting, then 16 bytes per posting + 4 per document while sorting, then the encoder's. What does not fit is DS2I_ENOMEM with
 * everything released (there is no chunked form). An index holds no wand data: ds2i_remap_wand (ds2i_build.h) renumbers that.
 * device_ms: extraction + map + sort + encoder. */
void ds2i_hip_remap_class_bounds(uint32_t bounds[3]);
int ds2i_hip_remap_postings(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                            const uint32_t* freqs, const uint32_t* doc_map, uint32_t* out_docs, uint32_t* out_freqs, double* device_ms);
int ds2i_hip_remap_index(int device, int from_kind, const void* image, size_t bytes, const uint32_t* doc_map, uint64_t map_len, int to_kind,
                         ds2i_blob** out_image, double* device_ms);
/* Diagnostic: the hipEvent milliseconds of this thread's last ds2i_hip_remap_postings / ds2i_hip_remap_index: ms[0] the map kernel,
 * ms[1 .. 3] sort classes 1, 2 and 3, ms[4] the extraction and ms[5] the encoder (both 0 for ds2i_hip_remap_postings). */
void ds2i_hip_remap_ms(double ms[6]);

/* Merging indexes on the GPU: nsrc >= 1 images (any of the nine kinds, each its own) become the image of to_kind of the merged
 * collection, byte-identical to the host builder's over ds2i_merge_postings' lists (ds2i_build.h, the host twin, which states the
 * semantics of the two maps: doc_map NULL = base + old doc-id, term_map NULL = the identity). nlists: the merged number of lists;
 * 0: the smallest that holds every mapped term.
 *
 * ds2i_hip_merge_indexes. Checks, in this order, all before a device is looked for: null arguments and nsrc == 0 (DS2I_EINVAL), the
 * kinds (to_kind as ds2i_hip_convert_index takes it: DS2I_BLOCK_QMX and DS2I_BLOCK_MIXED are DS2I_EINVAL, same message, before any
 * image is read), the host parse of every image (DS2I_EFORMAT), then the twin's checks of the maps (DS2I_EINVAL), then the device.
 * The host plans, from the list lengths alone, where every source list's run starts inside its merged list (runs lie in source
 * order). Then each source in turn: bare upload, extraction, the image closed, one placement kernel that reads the source's postings
 * coalesced and stores each at its place with its doc-id mapped, the source's postings freed. A doc-id at or past a source's map
 * is found by that kernel, which reads nothing past the map: DS2I_EFORMAT. If the concatenated doc maps are not the identity every
 * merged list is sorted by the segmented sort of ds2i_hip_remap_postings; with all-default maps nothing is sorted and no second buffer
 * pair is allocated. Then the encoder over the postings where they lie. Peak device memory: the merged postings (8 bytes each) plus
 * one source's image and postings, then the sort's or the encoder's. What does not fit is DS2I_ENOMEM with everything released.
 * An index holds no wand data and none is merged. device_ms: extraction + placement + sort + encoder.
 *
 * ds2i_hip_merge_postings: the same placement and sort over sources in CSR form on the host; the merged collection comes back as
 * ds2i_merge_postings returns it, element for element. Checks: the twin's, then the device. */
typedef struct ds2i_merge_source {
    int kind;
    const void* image;
    size_t bytes;
    const uint32_t* doc_map;
    uint64_t map_len;
    const uint32_t* term_map;
    uint64_t terms_len;
} ds2i_merge_source;
typedef struct ds2i_merge_postings_source ds2i_merge_postings_source; /* ds2i_build.h */
int ds2i_hip_merge_indexes(int device, const ds2i_merge_source* src, uint32_t nsrc, uint64_t nlists, int to_kind, ds2i_blob** out_image,
                           double* device_ms);
int ds2i_hip_merge_postings(int device, const ds2i_merge_postings_source* src, uint32_t nsrc, uint64_t nlists, uint64_t* num_docs,
                            uint64_t* out_nlists, ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs, double* device_ms);
/* Diagnostic: the hipEvent milliseconds of this thread's last merge: ms[0] the extractions, ms[1] the placement kernels, ms[2] sort
 * classes 1 to 3 summed, ms[3] the encoder (ms[0] and ms[3] are 0 for ds2i_hip_merge_postings); ms[4 .. 7] are 0. */
void ds2i_hip_merge_ms(double ms[4 + 4]);

/* Splitting an index on the GPU, the inverse of a merge: an image becomes nshards >= 1 images, one per shard of its documents, each with
 * the doc map and the term map that ds2i_hip_merge_indexes takes. shard_of[d] is the shard of document d, < nshards, or
 * DS2I_SPLIT_DROP (ds2i_build.h) to delete the document. ds2i_split_postings (ds2i_build.h, the host twin) states the semantics:
 * order-preserving local doc-ids, lists without a posting in the shard dropped, nothing sorted. With no document dropped, merging the
 * shards with their maps gives the input back, byte for byte when the kinds agree. An index holds no wand data: ds2i_split_wand
 * (ds2i_build.h) makes a shard's under the collection's normalisation, ds2i_hip_index_set_collection_stats gives an open shard the
 * collection's BM25 statistics, and ds2i_hip_shard_set_* below queries the shards as one index, in the collection's doc-ids.
 *
 * A shard's postings are the stable compaction of the source postings by the flag shard_of[doc-id] == shard. The source postings are
 * cut into windows of ds2i_hip_split_window() postings. Per shard: a count kernel (kept postings per window, a ballot and a popcount
 * per 64 postings), the exclusive scan of the window counts on the host (u64), a scatter kernel (a wavefront walks a window from its
 * scanned position; doc-ids become local ids through a table computed once on the host) and an offsets kernel (the kept postings
 * before every source list start; lists whose two consecutive values are equal vanish). A launch has at most
 * ds2i_hip_split_grid_waves(compute units) wavefronts, which stride over the windows. Each shard costs one more read of the source
 * postings; there is no single pass for all shards.
 *
 * ds2i_hip_split_index: an image of from_kind (any of the nine) in, *shards = nshards ds2i_split_shard out (num_docs, nlists, image,
 * doc_map, term_map; free with ds2i_split_free): every image is byte-identical to the host builder's image of to_kind over the twin's
 * lists for that shard. Checks, in this order, all before a device is looked for: null arguments and nshards == 0 (DS2I_EINVAL), the
 * kinds (to_kind as ds2i_hip_convert_index takes it: DS2I_BLOCK_QMX and DS2I_BLOCK_MIXED are DS2I_EINVAL, same message, before the
 * image is read), the host parse of the image (DS2I_EFORMAT), map_len == the image's number of documents, the values of shard_of (the
 * first that is neither a shard nor the drop value is named), the first shard that is assigned no document (DS2I_EINVAL), then the
 * device. Then: bare upload, extraction, the image closed, shard_of and the local ids uploaded once, and every shard in turn: count,
 * scan, buffers of exactly the shard's size, scatter, offsets, the encoder over the postings where they lie (it frees them). A shard
 * that has documents but receives no posting is found when it is counted: DS2I_EINVAL ("List must be nonempty", the shard named),
 * everything released, no output written. The source postings are freed after the last shard. Peak device memory: the source postings
 * (8 bytes each; the image beside them while extracting) plus 8 bytes per document, 16 per list and 12 per window, plus one shard's
 * postings and the encoder's. What does not fit is DS2I_ENOMEM with everything released. device_ms: extraction + count + offsets +
 * scatter + encoder.
 *
 * ds2i_hip_split_postings: the same kernels over a collection in CSR form on the host; the shards come back as ds2i_split_postings
 * returns them, element for element (a shard may hold no document or no list). Checks: the twin's, then the device. A doc-id >=
 * num_docs among the postings is found by the count kernel, which never reads past shard_of: DS2I_EFORMAT, no output written. */
typedef struct ds2i_split_shard ds2i_split_shard; /* ds2i_build.h */
/* The number of documents and of lists of an image, from the host parse alone (what ds2i_hip_split_index checks map_len against): no
 * device is looked for. A caller that cuts doc-id ranges needs it to write shard_of. Null arguments and an unknown kind are DS2I_EINVAL,
 * an image that does not parse DS2I_EFORMAT; on an error nothing is written. */
int ds2i_hip_image_shape(int index_kind, const void* image, size_t bytes, uint64_t* num_docs, uint64_t* nlists);
uint32_t ds2i_hip_split_window(void);
uint32_t ds2i_hip_split_grid_waves(uint32_t compute_units);
int ds2i_hip_split_index(int device, int from_kind, const void* image, size_t bytes, const uint32_t* shard_of, uint64_t map_len,
                         uint32_t nshards, int to_kind, ds2i_split_shard** shards, double* device_ms);
int ds2i_hip_split_postings(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                            const uint32_t* freqs, const uint32_t* shard_of, uint32_t nshards, ds2i_split_shard** shards, double* device_ms);
/* Diagnostic: the hipEvent milliseconds of this thread's last split, summed over its shards: ms[0] the extraction, ms[1] the count
 * kernels, ms[2] the offsets kernels, ms[3] the scatter kernels, ms[4] the encoder (ms[0] and ms[4] are 0 for
 * ds2i_hip_split_postings); ms[5 .. 7] are 0. */
void ds2i_hip_split_ms(double ms[8]);

/* Indexing documents on the GPU: a forward collection (documents as sequences of term ids, what a tokenizer emits) inverted into posting
 * lists or into an index image, and the same operation run the other way, the forward index of an image. Both are one primitive, the
 * transposition of a sparse matrix in CSR form. ds2i_invert_documents and ds2i_transpose_postings (ds2i_build.h, the host twins) state
 * the semantics; every answer is unique and the device returns the twins' arrays element for element.
 *
 * The plan. (1) The tokens are copied up and staged as keys with a payload of 1; the stage kernel flags a token >= nterms, which is
 * DS2I_EFORMAT with nothing written. (2) Every document is sorted by the segmented sort of ds2i_hip_remap_postings (segments = the
 * documents, key bound = nterms). (3) Run-length compaction in windows of ds2i_hip_invert_window() tokens: an entry starts wherever the
 * term differs from the previous token's or a document starts; a count kernel (a ballot and a popcount per 64 tokens), the scan of the
 * window counts on the host (u64), a scatter kernel that writes (term, freq = the run's length; a run may span any number of windows)
 * and an offsets kernel (the entries before every document start) give the forward index in canonical form. (4) The transposition: a
 * histogram of the columns, its scan on the host, a scatter that takes each entry's place from a per-column cursor with a returning
 * atomic add, and the segmented sort again (segments = the columns, key bound = nrows) to put every column in row order. All adds to
 * one column's cursor serialise: a term present in every document costs one returning add per document on one word. (5) The encoder and
 * the wand kernel over the postings where they lie, from one staging, as ds2i_hip_build_collection; the Elias-Fano kinds come down once
 * for the host planner, as in a conversion. No kernel waits for another workgroup; a launch has at most ds2i_hip_split_grid_waves(compute
 * units) wavefronts, which stride over the windows.
 *
 * Device memory: 8 bytes per token while sorting the documents, 16 if any document is longer than the class-2 bound of
 * ds2i_hip_remap_class_bounds; then the tokens beside the forward entries (8 bytes each) and 16 bytes per document and 12 per window of
 * tables; then the forward entries beside the transposed entries (8 bytes each) and 8 bytes per row and 12 per column; then the
 * transposed entries and the second sort's scratch (8 bytes per entry more if a list is longer than the class-2 bound); then the
 * encoder's. What does not fit is DS2I_ENOMEM with everything released. There is no chunked form.
 *
 * Checks of every entry point, in the twins' order, all before anything is staged: null arguments and the offsets; 2^32 documents or
 * terms (rows or columns), or more; a document (row) of 2^32 tokens (entries) or more (all DS2I_EINVAL); then the device (DS2I_EDEVICE).
 * No output -- device_ms included -- is written on any error.
 *
 * ds2i_hip_invert_postings: ds2i_invert_documents' outputs (lists for all nterms terms, empty ones included, and doc_sizes).
 * ds2i_hip_transpose_postings: ds2i_transpose_postings' outputs. A column >= ncols, or columns that do not strictly increase within a
 * row, are found by the count kernel, which indexes nothing by them: DS2I_EFORMAT.
 * ds2i_hip_invert_documents: the image of index_kind over the twin's NONEMPTY lists, byte-identical to the host builder's; terms that
 * never occur vanish and term_map (u32, strictly increasing) gives the old term of every surviving list: the map ds2i_hip_merge_indexes
 * takes, so that a batch of new documents is indexed here and merged there with the default doc map. wand_image (may be NULL: none is
 * built) is byte-identical to ds2i_wand_* over the same lists with doc_sizes (u32[num_docs], every document's token count, the ds2i
 * .sizes value). index_kind: a kind ds2i_hip_encode_index writes; DS2I_BLOCK_QMX and DS2I_BLOCK_MIXED are DS2I_EINVAL with
 * ds2i_hip_convert_index's message, checked before anything else is read. Documents without a single token are DS2I_EINVAL ("List must
 * be nonempty").
 * ds2i_hip_forward_index: the forward index of an image of any of the nine kinds: document d holds terms[doc_offsets[d] ..
 * doc_offsets[d + 1]) (list numbers, strictly increasing) with freqs beside them; what a document-reordering method needs to make a map
 * for ds2i_hip_remap_index. Host parse (DS2I_EFORMAT), the device, bare upload, extraction, the image closed, transposition.
 * device_ms: the sum of ds2i_hip_invert_ms. */
uint32_t ds2i_hip_invert_window(void);
int ds2i_hip_invert_postings(int device, uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms,
                             ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs, ds2i_blob** doc_sizes, double* device_ms);
int ds2i_hip_transpose_postings(int device, uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets, const uint32_t* cols,
                                const uint32_t* vals, ds2i_blob** col_offsets, ds2i_blob** rows, ds2i_blob** out_vals, double* device_ms);
int ds2i_hip_invert_documents(int device, int index_kind, uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens,
                              uint64_t nterms, ds2i_blob** index_image, ds2i_blob** wand_image, ds2i_blob** term_map, ds2i_blob** doc_sizes,
                              double* device_ms);
int ds2i_hip_forward_index(int device, int index_kind, const void* image, size_t bytes, uint64_t* num_docs, uint64_t* nterms,
                           ds2i_blob** doc_offsets, ds2i_blob** terms, ds2i_blob** freqs, double* device_ms);
/* Diagnostic: the hipEvent milliseconds of this thread's last call of the four: ms[0] the check (stage) kernel, ms[1] the document
 * sort, ms[2] the mark and count kernels, ms[3] the scatter and offsets kernels, ms[4] the transposition's count and scatter kernels,
 * ms[5] the column sort, ms[6] the extraction (ds2i_hip_forward_index), ms[7] the encoder and the wand kernel
 * (ds2i_hip_invert_documents). Unused slots are 0. */
void ds2i_hip_invert_ms(double ms[8]);

/* Ordering documents on the GPU: the doc-id map of recursive graph bisection, the map ds2i_hip_remap_index takes. ds2i_order_postings
 * (ds2i_build.h, the host twin) states the algorithm; the result is made of integers alone, and the device returns the twin's doc_map
 * and trace element for element.
 *
 * The plan. The lists lie on the device as entries named by p0, a document's position at the level's start, every list in p0 order:
 * at level 0 that is the input, at every later level the entries go through the previous level's inverse and the segmented sort of
 * ds2i_hip_remap_postings orders every list again. A term's documents of one level segment are then one run of its list, and the
 * run's two degrees live at its first entry: no forward index is built. Once a level a runs kernel finds every entry's run by two
 * binary searches in its own list. Once an iteration: a degrees kernel (one atomic add per run and wavefront step), a gains kernel
 * (the term cost per entry from the uploaded LOGQ table, a 64-bit integer atomic add per entry into its document's gain), a keys
 * kernel ((order-reversing u32 image of the clamped gain, p0) per slot), the segmented sort over the 2^(l+1) halves with the full
 * 32-bit key bound, and a swap kernel (a thread per pair; the exchanges counted into one word the host reads). Where a half is longer
 * than the class-2 bound of ds2i_hip_remap_class_bounds the sort by gain is only stable, so the halves are sorted by p0 first (LSD:
 * p0, then gain); shorter halves compare whole (key, p0) pairs. Only integers are added, so no result depends on the order of the
 * atomics. No logarithm is evaluated on the device and no float is touched.
 *
 * Device memory: 16 bytes per posting (24 while a level's lists are sorted, if one is longer than the class-2 bound) and 40 bytes per
 * document (48 and the sort's tables while the halves are sorted). What does not fit is DS2I_ENOMEM naming these figures, with
 * everything released.
 *
 * Checks, all before any device is looked for. ds2i_hip_order_postings: ds2i_order_postings' checks in its order. ds2i_hip_order_index:
 * null arguments; an unknown index kind (any of the nine is taken); the image (host parse, DS2I_EFORMAT); num_docs >= 2^32 - 2; the
 * parameters. Then the device (DS2I_EDEVICE). A doc-id >= num_docs among an image's postings is DS2I_EFORMAT from the check kernel.
 * No output -- device_ms included -- is written on any error.
 * ds2i_hip_order_index is the extraction followed by the ordering; the postings stay on the device. */
typedef struct ds2i_order_params ds2i_order_params; /* ds2i_build.h */
int ds2i_hip_order_postings(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                            const ds2i_order_params* params, ds2i_blob** doc_map, ds2i_blob** trace, double* device_ms);
int ds2i_hip_order_index(int device, int index_kind, const void* image, size_t bytes, const ds2i_order_params* params, ds2i_blob** doc_map,
                         ds2i_blob** trace, double* device_ms);
/* Diagnostic: the hipEvent milliseconds of this thread's last call of the two: ms[0] the extraction (ds2i_hip_order_index), ms[1] the
 * renumbering and sort of the lists at every level's start but the first, ms[2] the check, level-start and runs kernels, ms[3] the
 * degrees kernels, ms[4] the gains kernels, ms[5] the keys kernels and the sorts of the halves, ms[6] the swap kernels, ms[7] the
 * compose kernels and the final map. device_ms is their sum. */
void ds2i_hip_order_ms(double ms[8]);

/* Querying document shards as one index. A collection cut by ds2i_hip_split_index answers a query batch as the whole collection would,
 * in the collection's doc-ids, from three parts: the collection's BM25 statistics on every shard (ds2i_hip_index_set_collection_stats),
 * every shard's wand data under the collection's normalisation (ds2i_split_wand, ds2i_build.h), and a merge of the shards' top-k rows.
 *
 * ds2i_hip_merge_topk: the device form of ds2i_merge_topk (ds2i_build.h, the host twin, which states the key order and the checks; all
 * of them are made before a device is looked for). All pointers are host pointers: the rows and the maps go up, one kernel merges, the
 * result comes down. The kernel takes one wavefront per query, and wavefronts stride over the queries (at most
 * ds2i_hip_merge_topk_grid(compute units, k) of them: as many workgroups of one wavefront as a compute unit's LDS and its 32 wavefront
 * slots hold at that k, 5 at k = 1024 and 32 from k = 128 down). A row arrives sorted by score with its equal-score runs in LOCAL id order, which
 * under an increasing doc_map is key order; the host marks the row sets whose map is not increasing, and such a row is first sorted by
 * key in LDS (a bitonic network over at most 1024 keys). Rows are then folded one at a time into a best-k buffer in LDS: both sides
 * are sorted, an element's rank in the union is its own position plus a binary search in the other side (lower bound one way, upper
 * bound the other: ranks stay distinct on duplicate keys), and elements of rank < k are stored at their rank. No atomics; three
 * buffers of 8 * (k rounded up to a power of two) bytes of dynamic LDS. device_ms (may be NULL): the hipEvent time of the kernel. */
#define DS2I_HIP_MAX_SHARDS 64
struct ds2i_topk_rows; /* ds2i_build.h */
int ds2i_hip_merge_topk(int device, const struct ds2i_topk_rows* rows, uint32_t nrows, uint32_t nq, uint32_t k, float* out_scores,
                        uint32_t* out_docs, uint32_t* out_lens, double* device_ms);
uint32_t ds2i_hip_merge_topk_grid(uint32_t compute_units, uint32_t k);

/* The shard set: nshards sources, each an index image of its own kind on its own device with the maps of a split.
 * open. Checks, in this order, all before a device is looked for: null arguments (DS2I_EINVAL); nshards == 0 or above
 * DS2I_HIP_MAX_SHARDS; the kinds; every image through the host parse (DS2I_EFORMAT, as ds2i_hip_image_shape gives); map_len and
 * terms_len against the parsed shape; every term map strictly increasing and < collection_terms; every doc map < collection_docs with
 * no id taken twice across the whole set (one bit per document, the first offender named). Statistics: stats_num_docs == 0 means the
 * sum of the shards' documents; stats_df == NULL means, per collection term, the sum of the lengths of the shard lists mapped to it, so
 * that a set made from a split with nothing dropped scores exactly as the unsplit index; a given stats_df (collection_terms entries)
 * must be at least that sum and at most stats_num_docs, per term (DS2I_EINVAL, the term named). Then every shard that has lists and
 * documents is opened with ds2i_hip_index_open on its device and given its statistics; a shard with no lists or no documents is
 * accepted and skipped. wand_image NULL: the shard answers `and` / `or` only (a ranked operator is DS2I_ENOWAND). The merge runs on the
 * device of the first opened shard, where the doc maps are kept. The images and maps are not referenced after the call.
 * query: op is one of the four ranked operators (DS2I_OP_TOPK_DOCS is implied and accepted) or DS2I_OP_AND / DS2I_OP_OR.
 * DS2I_OP_AND_FREQ, DS2I_OP_OR_FREQ, DS2I_OP_REFERENCE_ORDER and, for a ranked operator, k == 0 or k > DS2I_HIP_MAX_K_LONG are
 * DS2I_EINVAL; a term >= collection_terms is DS2I_ETERM. Per shard the queries are translated on the host by a binary search in the
 * term map: repeats are kept (they are the query term frequencies); for `and` and `ranked_and` a query with a distinct term absent from
 * the shard is sent as the empty query; for the union operators absent terms are dropped. The shards' batches are submitted together,
 * each through a pipeline of its own, and collected; the rows come back through the public fetch and go up to the merge device, where
 * ds2i_hip_merge_topk's kernel merges them. Ranked: out_topk / out_topk_docs (nq * k each, collection doc-ids) and out_topk_len (nq) are
 * the merged rows, out_count[q] the merged row's length (out_count and out_topk_len may be NULL). and / or: out_count[q] is the sum of the
 * shards' counts and no other output is touched.
 * Ties: if every doc map is increasing, the set breaks ties as the whole index does. Otherwise a tie at a shard's own k-th place is
 * broken by that shard's local ids; the merge still orders by collection id.
 * stats (may be NULL): per source its batch's kernel_ms (0 for a skipped shard), the merge kernel's ms, and the host milliseconds of the
 * translation. A set is not re-entrant. */
typedef struct ds2i_shard_source {
    int device, kind;
    const void* image;      size_t bytes;
    const void* wand_image; size_t wand_bytes;   /* ds2i_split_wand's; NULL: the and / or counts only */
    const uint32_t* doc_map;  uint64_t map_len;  /* local -> collection doc-id, injective */
    const uint32_t* term_map; uint64_t terms_len;/* local -> collection term, strictly increasing */
} ds2i_shard_source;
typedef struct ds2i_hip_shard_stats {
    double kernel_ms[DS2I_HIP_MAX_SHARDS];
    double merge_ms, translate_ms;
    uint32_t shards_open;
} ds2i_hip_shard_stats;
typedef struct ds2i_hip_shard_set ds2i_hip_shard_set;
int ds2i_hip_shard_set_open(const ds2i_shard_source* src, uint32_t nshards, uint64_t collection_docs, uint64_t collection_terms,
                            uint64_t stats_num_docs, const uint32_t* stats_df, ds2i_hip_shard_set** out);
int ds2i_hip_shard_set_query(ds2i_hip_shard_set* s, int op, uint32_t k, const uint32_t* terms, const uint32_t* query_offsets,
                             uint32_t nq, uint64_t* out_count, float* out_topk, uint32_t* out_topk_docs, uint32_t* out_topk_len,
                             ds2i_hip_shard_stats* stats);
void ds2i_hip_shard_set_close(ds2i_hip_shard_set* s);

/* Inspection of the upload-time pruning tables of one list (test hooks; both tables exist only with wand data).
 * block weights: bmw[b] = max over block b's postings of bm25::doc_term_weight(freq, norm_len[doc]) (the block-level
 * analogue of wand_data's max_term_weight, wand_data.hpp:40-52); out gets *nblocks floats (capacity in floats).
 * range table, level 1..3: byte e covers the doc-ids [e << *shift, (e + 1) << *shift): 0 = no posting of the list there,
 * else entry * (*list_max / 255) >= the largest doc_term_weight of the range; level l + 1 halves the resolution six
 * times (its entry e is the maximum of entries 64 e .. 64 e + 63 of level l). out gets *entries bytes. A table that
 * was not built (no wand data, DS2I_NO_BMW / DS2I_NO_RMW) reports 0 entries.
 * level 4: the membership hints, one byte per level-1 entry: 0 = the range holds no posting, 255 = two or more, else
 * 1 + (offset of its one posting inside the range) mod 254 (block_optpfor indexes; 0 entries elsewhere). */
int ds2i_hip_list_block_weights(ds2i_hip_index* idx, uint32_t term, float* out, uint64_t capacity, uint64_t* nblocks);
int ds2i_hip_list_range_table(ds2i_hip_index* idx, uint32_t term, uint32_t level, uint8_t* out, uint64_t capacity,
                              uint64_t* entries, uint32_t* shift, float* list_max);

/* profiling aid: streams the whole index arena once with the decoders' load shape (calibrates FETCH_SIZE) */
int ds2i_hip_calibration_read(ds2i_hip_index* idx, uint64_t* bytes_read);
/* GPU unit-test hook: wave64 inclusive prefix sum over rows of 64 values */
int ds2i_hip_selftest_scan(int device, const uint32_t* in, uint32_t* out, uint32_t rows);
/* GPU unit-test hook: the kernels' bm25::doc_term_weight (bm25.hpp:11-15), element-wise */
int ds2i_hip_selftest_bm25(int device, const uint32_t* freqs, const float* norm_lens, float* out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
