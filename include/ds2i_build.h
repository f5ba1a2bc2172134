/* ds2i_build.h -- host-side (CPU) index construction entry points of libds2i_hip.so.
 *
 * These replace the build-side tools the benchmark loop needs because the reference cannot be
 * compiled here (create_freq_index.cpp:45-110, create_wand_data.cpp:8-29,
 * block_freq_index::builder block_freq_index.hpp:18-70). They produce the reference's on-disk
 * images (block_freq_index / wand_data) that ds2i_hip_index_open consumes. Nothing here is on
 * the timed query path and nothing here touches the GPU: the GPU forms of the encoder, of the
 * block_mixed optimiser and of the wand_data builder (ds2i_hip_encode_index, ds2i_hip_hybrid_analyse /
 * _freeze, ds2i_hip_build_wand, ds2i_hip_build_collection) are in ds2i_hip.h.
 */
#ifndef DS2I_BUILD_H
#define DS2I_BUILD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ds2i_builder ds2i_builder;
typedef struct ds2i_blob ds2i_blob; /* owned byte buffer returned by the builders */

/* Synthetic Zipf collection; every list is a pure function of (seed, term). */
typedef struct ds2i_synth_params {
    uint64_t seed;
    uint32_t num_docs;
    uint32_t num_terms;
    double zipf_exp;          /* list length(rank r) = max(min_len, top_df_frac*N*r^-zipf_exp) */
    double top_df_frac;
    uint32_t min_len;
    uint32_t clustered_every; /* every k-th list alternates dense/sparse segments; 0 = never */
    /* correlated terms (both 0: independent lists): documents come in runs of 4096 doc-ids of one of `topics` topics, every
     * term has a home topic and is topic_boost times as likely in its documents (list lengths unchanged) */
    uint32_t topics;
    uint32_t topic_boost;
} ds2i_synth_params;

const uint8_t* ds2i_blob_data(const ds2i_blob* b);
size_t ds2i_blob_size(const ds2i_blob* b);
void ds2i_blob_free(ds2i_blob* b);

/* block_freq_index<Codec>::builder (block_freq_index.hpp:18-70) for kinds 0..4, freq_index<...>::builder
 * (freq_index.hpp:19-94) for kinds 5..8; codec = enum ds2i_hip_index_kind */
int ds2i_builder_create(int codec, uint64_t num_docs, ds2i_builder** out);
int ds2i_builder_add_posting_list(ds2i_builder* b, uint64_t n, const uint32_t* docs, const uint32_t* freqs);
int ds2i_builder_freeze(ds2i_builder* b, ds2i_blob** image); /* succinct::mapper::freeze image */
void ds2i_builder_free(ds2i_builder* b);

/* wand_data<bm25> (wand_data.hpp:20-52): sizes = doc lengths; lists are streamed in term order */
typedef struct ds2i_wand_builder ds2i_wand_builder;
int ds2i_wand_create(const uint32_t* doc_sizes, uint64_t num_docs, ds2i_wand_builder** out);
int ds2i_wand_add_list(ds2i_wand_builder* w, uint64_t n, const uint32_t* docs, const uint32_t* freqs);
int ds2i_wand_freeze(ds2i_wand_builder* w, ds2i_blob** image);
void ds2i_wand_free(ds2i_wand_builder* w);

/* single block encoders (test hooks for the codec round trips of test_block_codecs.cpp:9-46).
 * sum_of_values == 0xFFFFFFFF means "unknown" like the reference. Returns a blob. */
int ds2i_encode_block(int codec, const uint32_t* values, uint32_t sum_of_values, uint32_t n, ds2i_blob** out);
int ds2i_encode_vbyte(uint32_t value, ds2i_blob** out);
/* bm25::query_term_weight / doc_term_weight (bm25.hpp:11-24), element-wise, as the host side of the query path
 * computes them (float32) */
int ds2i_bm25_query_term_weight(const uint64_t* qtf, const uint64_t* df, uint64_t num_docs, uint64_t n, float* out);
int ds2i_bm25_doc_term_weight(const uint64_t* freq, const float* norm_len, uint64_t n, float* out);
int ds2i_encode_posting_list(int codec, uint32_t n, const uint32_t* docs, const uint32_t* freqs, ds2i_blob** out);

/* One sequence of the Elias-Fano family written on its own into a fresh bit string (test hook for the reference's
 * layout tests test_compact_elias_fano.cpp:45-80, test_compact_ranked_bitvector.cpp:36-68,
 * test_partitioned_sequence.cpp:13-111, test_uniform_partitioned_sequence.cpp). seq_kind: */
enum ds2i_sequence_kind {
    DS2I_SEQ_ELIAS_FANO = 0,       /* compact_elias_fano */
    DS2I_SEQ_RANKED_BITVECTOR = 1, /* compact_ranked_bitvector (strictly increasing values) */
    DS2I_SEQ_INDEXED = 2,          /* indexed_sequence: 1 type bit + the cheapest of EF / ranked bitvector / all-ones */
    DS2I_SEQ_STRICT = 3,           /* strict_sequence */
    DS2I_SEQ_PARTITIONED_INDEXED = 4, /* partitioned_sequence<indexed_sequence> */
    DS2I_SEQ_PARTITIONED_STRICT = 5,  /* partitioned_sequence<strict_sequence> */
    DS2I_SEQ_UNIFORM_INDEXED = 6,     /* uniform_partitioned_sequence<indexed_sequence> */
    DS2I_SEQ_UNIFORM_STRICT = 7       /* uniform_partitioned_sequence<strict_sequence> */
};
/* params = {ef_log_sampling0, ef_log_sampling1, rb_log_rank1_sampling, rb_log_sampling1, log_partition_size}
 * (global_parameters.hpp:5-31; NULL = defaults). bits = the image as little-endian u64 words, *nbits its length. */
int ds2i_write_sequence(int seq_kind, const uint64_t* values, uint64_t n, uint64_t universe, const uint8_t params[5],
                        ds2i_blob** bits, uint64_t* nbits);

/* The partition end points the DS2I_OPT builder chooses (optimal_partition, the (1+eps)-approximate shortest path) for every
 * list of a collection in CSR form (list t = docs / freqs [list_offsets[t], list_offsets[t+1]); doc-ids strictly increasing and
 * < num_docs, freqs >= 1, lists nonempty, else DS2I_EINVAL). Per side -- docs: the doc-ids over num_docs; freqs: the strict prefix
 * sums of the freqs over occurrences + 1 -- *_ends = the exclusive end index of every partition of every list back to back (u32),
 * *_offs = nlists + 1 u64 offsets into it. List-parallel on at most 16 threads. The reference of ds2i_hip_opt_partition. */
int ds2i_opt_partition(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                       ds2i_blob** docs_ends, ds2i_blob** docs_offs, ds2i_blob** freqs_ends, ds2i_blob** freqs_offs);

/* Renumbering the documents of a collection: new doc-id = doc_map[old doc-id], doc_map a permutation of [0, num_docs). Deleting
 * documents (a map that drops ids) is ds2i_split_postings' work, below. The device forms, ds2i_hip_remap_postings and ds2i_hip_remap_index, are in ds2i_hip.h.
 * check_doc_map: DS2I_OK, or DS2I_EINVAL with ds2i_hip_last_error() naming the FIRST offending old doc-id: one whose value is
 * >= num_docs, or the second document sent to an id already taken. One bit per document; every entry point that takes a map runs it
 * before anything else is done with the map, and before any device is touched.
 * remap_postings: the host twin of ds2i_hip_remap_postings, in place: lists in the CSR form of ds2i_opt_partition (empty lists are
 * allowed), every doc-id through the map, then every list sorted by its new doc-ids, the freqs travelling with them; list lengths and
 * list order do not change. Lists are spread over `threads` host threads (<= 0: up to 16). A doc-id >= num_docs among the postings
 * is DS2I_EFORMAT, as on the device; lists already done stay remapped.
 * remap_wand: the wand image of the renumbered collection with no pass over the postings: norm_lens permuted, max_term_weight
 * copied. Byte-identical to ds2i_wand_create / _add_list / _freeze over the renumbered collection: the average document length is a
 * sum of integer-valued floats in a double, which does not depend on their order, and a term's maximum is taken over the same
 * floats. num_docs is the map's length and must be the image's. */
int ds2i_check_doc_map(const uint32_t* doc_map, uint64_t num_docs);
int ds2i_remap_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, uint32_t* docs, uint32_t* freqs,
                        const uint32_t* doc_map, int threads);
int ds2i_remap_wand(const void* wand_image, size_t bytes, const uint32_t* doc_map, uint64_t num_docs, ds2i_blob** out);

/* Merging collections: nsrc >= 1 sources become one. Source s holds num_docs documents and nlists lists in the CSR form of
 * ds2i_opt_partition (empty lists are allowed) and optionally two maps. doc_map (map_len == num_docs entries) gives the merged doc-id
 * of each of its documents; NULL: base + old doc-id, base the documents of the earlier sources. The maps, defaults filled in and
 * concatenated in source order, must be a permutation of all documents (what ds2i_check_doc_map checks). term_map (terms_len == nlists
 * entries, strictly increasing, < the merged number of lists) gives the merged term of each of its lists; NULL: the identity. The
 * merged list of a term is the union of the mapped postings of every source list sent to it, sorted by doc-id, the freqs travelling
 * with their postings; doc-ids are distinct across sources, so it is unique. Every merged term must receive a list.
 * merge_postings: the host twin of ds2i_hip_merge_postings (ds2i_hip.h). nlists: the merged number of lists; 0: the smallest that holds
 * every mapped term. Checks, all DS2I_EINVAL, in this order: null arguments and the offsets; no source; 2^32 documents or lists; a map
 * of the wrong length; the concatenated doc maps; a term map that does not increase or leaves the merged lists; the first merged
 * term that receives no list ("List must be nonempty", as the builders say). A doc-id >= num_docs among a source's postings is
 * DS2I_EFORMAT. Out: *num_docs, list_offsets u64[*out_nlists + 1], docs / freqs u32[postings]; free each with ds2i_blob_free; on an
 * error nothing is written. At most 16 host threads (threads <= 0: up to 16). */
typedef struct ds2i_merge_postings_source {
    uint64_t num_docs, nlists;
    const uint64_t* list_offsets;
    const uint32_t *docs, *freqs;
    const uint32_t* doc_map;
    uint64_t map_len;
    const uint32_t* term_map;
    uint64_t terms_len;
} ds2i_merge_postings_source;
int ds2i_merge_postings(const ds2i_merge_postings_source* src, uint32_t nsrc, uint64_t nlists, int threads, uint64_t* num_docs,
                        uint64_t* out_nlists, ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs);

/* Splitting a collection by documents, the inverse of a merge: shards and deletions. The collection holds num_docs documents and nlists
 * lists in the CSR form of ds2i_opt_partition (empty lists are allowed). shard_of[d] (num_docs entries) is the shard of document d,
 * < nshards, or DS2I_SPLIT_DROP to delete the document. Shard s holds the documents d with shard_of[d] == s in increasing old id: the
 * local id of a document is its rank among them, and doc_map (u32[num_docs of the shard], strictly increasing) gives the old id of each.
 * A list survives in a shard if at least one of its postings lies in a document of the shard; surviving lists keep their relative
 * order, and term_map (u32[nlists of the shard], strictly increasing) gives the old term of each. The surviving postings of a list
 * keep their order, carry their local doc-ids and keep their freqs. Local ids preserve the order of the old ones, so nothing is
 * sorted; a caller who wants another order remaps the shard afterwards. doc_map and term_map are the maps ds2i_merge_postings and
 * ds2i_hip_merge_indexes take: with no document dropped and every input list nonempty, merging the shards with them gives the input
 * back. A shard may come back with no documents or with no lists.
 * Wand data and scores: an index holds no wand data; ds2i_split_wand (below) gives a shard the collection's own normalisation, and
 * ds2i_hip_index_set_collection_stats (ds2i_hip.h) the collection's number of documents and document frequencies, so that a shard
 * scores as the collection does; ds2i_hip_shard_set_* (ds2i_hip.h) queries the shards of a split as one index. A shard opened without
 * them scores by its own statistics, which are not the collection's.
 * split_postings: the host twin of ds2i_hip_split_postings (ds2i_hip.h). Checks, all DS2I_EINVAL, in this order: null arguments and the
 * offsets; nshards == 0; 2^32 documents or lists; the first document whose shard_of is neither < nshards nor the drop value (named). A
 * doc-id >= num_docs among the postings is DS2I_EFORMAT. Out: *shards = an array of nshards ds2i_split_shard whose members are blobs
 * (doc_map, term_map u32; list_offsets u64[nlists + 1]; docs / freqs u32[postings]; image is NULL here: it is ds2i_hip_split_index's);
 * free the array and all its blobs with one ds2i_split_free. On an error nothing is written. Lists are spread over at most 16 host
 * threads (threads <= 0: up to 16); every shard costs one pass over the postings. */
#define DS2I_SPLIT_DROP 0xFFFFFFFFu
typedef struct ds2i_split_shard {
    uint64_t num_docs, nlists;
    ds2i_blob *doc_map, *term_map;
    ds2i_blob *list_offsets, *docs, *freqs; /* the postings forms; NULL from ds2i_hip_split_index */
    ds2i_blob* image;                       /* ds2i_hip_split_index; NULL from the postings forms */
} ds2i_split_shard;
int ds2i_split_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                        const uint32_t* shard_of, uint32_t nshards, int threads, ds2i_split_shard** shards);
void ds2i_split_free(ds2i_split_shard* shards, uint32_t nshards);

/* A shard's wand data under the COLLECTION's normalisation, with no pass over the postings: norm_lens[i] = the collection's
 * norm_lens[doc_map[i]] (ndocs entries), max_term_weight[j] = the collection's max_term_weight[term_map[j]] (nterms entries); the maps
 * are a split's, and need not be increasing. This is on purpose NOT the image ds2i_wand_create gives over the shard: that one divides by
 * the shard's own average document length, and scores under it are not the collection's. The gathered maximum is an upper bound of the
 * maximum over the shard's own postings, which is all the pruning needs (the exact maximum is not computed). Checks, all DS2I_EINVAL:
 * null arguments (a map may be NULL when its length is 0); the first doc_map entry, then the first term_map entry, at or past the
 * image's arrays, named. An image that does not parse is DS2I_EFORMAT. On an error nothing is written.
 * wand_arrays: an image read back into its two float arrays (blobs of float32; either output may be NULL). */
int ds2i_split_wand(const void* wand_image, size_t bytes, const uint32_t* doc_map, uint64_t ndocs, const uint32_t* term_map, uint64_t nterms,
                    ds2i_blob** out);
int ds2i_wand_arrays(const void* wand_image, size_t bytes, ds2i_blob** norm_lens, ds2i_blob** max_term_weight);

/* Merging top-k rows: what several shards answered for the same nq queries with DS2I_OP_TOPK_DOCS becomes what the whole collection
 * answers. The semantics, in integers:
 *   - A candidate is entry i < lens[q] of row set r for query q.
 *   - Its key is the u64 ((0xFFFFFFFF - bits(score)) << 32) | g, with g = doc_map ? doc_map[doc] : doc and bits() the float's bit pattern.
 *   - The output row of q holds the min(k, sum over r of lens[q]) candidates of smallest key, in ascending key order: score descending,
 *     equal scores by collection doc-id ascending, and the smaller ids on a tie at the k-th place -- the rule DS2I_OP_TOPK_DOCS has for
 *     one index. out_lens[q] is that number.
 *   - Rows are padded as a single index pads them: -inf for scores, 0xFFFFFFFF for docs.
 *   - An input row is what DS2I_OP_TOPK_DOCS returns: sorted by score descending, equal scores by local doc-id ascending. The device
 *     form relies on it (this twin sorts every candidate and does not).
 * The bit pattern of a non-negative finite float orders as the float, and BM25 scores here are positive; the order is total and
 * integer, so ds2i_hip_merge_topk (ds2i_hip.h, the device form) and this twin agree element for element.
 * Checks, all DS2I_EINVAL, in this order (the device form makes them before a device is looked for): null arguments; nrows == 0 or
 * nrows > 64 (DS2I_HIP_MAX_SHARDS); k == 0 or k > 1024 (DS2I_HIP_MAX_K_LONG); the first lens[q] > k; the first candidate whose score has
 * its sign bit set or is not finite; the first candidate whose local id is >= map_len. Each names row set, query and position.
 * nq == 0 succeeds and writes nothing. Two candidates of one query with the same collection id are the caller's error: the result may
 * hold both, and nothing is read or written out of bounds because of it. At most 16 host threads (threads <= 0: up to 16). */
typedef struct ds2i_topk_rows {      /* what one shard answered for nq queries with DS2I_OP_TOPK_DOCS */
    const float* scores;             /* nq * k */
    const uint32_t* docs;            /* nq * k, local doc-ids */
    const uint32_t* lens;            /* nq, each <= k */
    const uint32_t* doc_map;         /* local -> collection doc-id; NULL: the ids are the collection's already */
    uint64_t map_len;
} ds2i_topk_rows;
int ds2i_merge_topk(const ds2i_topk_rows* rows, uint32_t nrows, uint32_t nq, uint32_t k, float* out_scores, uint32_t* out_docs,
                    uint32_t* out_lens, int threads);

/* Indexing documents: a forward collection inverted into posting lists, and the primitive behind it, the transposition of a sparse
 * matrix in CSR form. The host twins of ds2i_hip_invert_postings and ds2i_hip_transpose_postings (ds2i_hip.h), which return the same
 * arrays element for element.
 * A forward collection holds num_docs documents in CSR form: document d is tokens[doc_offsets[d] .. doc_offsets[d + 1]), each token a
 * term id < nterms, in any order, with repeats (what a tokenizer emits). Empty documents are allowed. num_docs and nterms are < 2^32 and
 * a document has < 2^32 tokens.
 * invert_documents: for every term t < nterms the documents that hold t: doc-ids strictly increasing, freq = the number of times t
 * occurs in the document; terms that never occur have empty lists. Out, as blobs: list_offsets u64[nterms + 1], docs / freqs
 * u32[postings], doc_sizes u32[num_docs] = every document's token count (the ds2i .sizes value). It is the canonical form of the
 * documents (every document's tokens sorted, equal neighbours turned into one (term, freq) entry) transposed.
 * transpose_postings: a CSR matrix of nrows rows whose column ids are strictly increasing within each row and < ncols, with one u32
 * value per entry, becomes the CSR of its transpose: col_offsets u64[ncols + 1], rows / out_vals u32[entries], the row ids strictly
 * increasing within each column and the values travelling along. transpose(transpose(x)) == x; the forward index of a collection
 * (every document's terms and freqs) is the transpose of its posting lists.
 * Checks, all DS2I_EINVAL, in this order: null arguments and the offsets (not starting at 0, or decreasing); 2^32 documents or terms
 * (rows or columns), or more; a document (row) of 2^32 tokens (entries) or more. Then a token >= nterms, or a column >= ncols or not
 * above its left neighbour in the row, is DS2I_EFORMAT and the message names the first offender. On an error nothing is written. The
 * work is spread over at most 16 host threads (threads <= 0: up to 16). */
int ds2i_invert_documents(uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms, int threads,
                          ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs, ds2i_blob** doc_sizes);
int ds2i_transpose_postings(uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets, const uint32_t* cols, const uint32_t* vals, int threads,
                            ds2i_blob** col_offsets, ds2i_blob** rows, ds2i_blob** out_vals);

/* Ordering documents: a doc-id map computed by recursive graph bisection (Dhulipala et al., KDD'16), the map ds2i_remap_postings and
 * ds2i_hip_remap_index take. Every codec here codes gaps, and an order that puts similar documents side by side makes the gaps small.
 * The input is the postings of a collection in the CSR form of ds2i_opt_partition without the freqs (empty lists are allowed; doc-ids
 * strictly increasing and < num_docs); the output is doc_map, u32[num_docs], a permutation with new id = doc_map[old id], and trace,
 * one u64 per (level, iteration) that ran: the exchanges of that iteration. Both are made of integers alone, and ds2i_hip_order_postings
 * (ds2i_hip.h) returns the same two arrays element for element.
 * Fixed point: LOGQ[x] = rint(log2((double)x) * 256) as u32, LOGQ[0] = 0. order_log_table writes LOGQ[0 .. n) to out.
 * Segments: level l cuts the positions into 2^l segments, segment k = [(k * num_docs) >> l, ((k + 1) * num_docs) >> l); its halves are
 * the level l + 1 segments 2k (left) and 2k + 1 (right). Level l runs iff l < max_levels and every level l + 1 segment holds at least
 * min_half documents; the first level that fails ends the run, and num_docs < 2 * min_half gives the identity.
 * State: order[s], the document at position s, starts as the identity. At a level's start every document is named by its position
 * then, p0, and members[s] = s. One iteration, of at most `iterations`: (1) for every term and level l segment, dl and dr, the term's
 * documents now in the left and the right half; (2) for every document the sum over its terms, as int64 clamped to int32, of
 *   c = da*(LOGQ[na]-LOGQ[da+1]) + db*(LOGQ[nb]-LOGQ[db+1]) - (da-1)*(LOGQ[na]-LOGQ[da]) - (db+1)*(LOGQ[nb]-LOGQ[db+2])
 * with na / nb the sizes of its own / the other half and da / db the term's degrees there: its gain; (3) each half's members sorted
 * by gain descending, equal gains by smaller p0 first; (4) in each segment, with m the smaller half's size, the i-th left and the i-th
 * right member exchanged for every i < m with gain_left[i] + gain_right[i] > 0; (5) zero exchanges end the level. At a level's end
 * order'[s] = order[members[s]]; at the end of the run doc_map[order[s]] = s.
 * params: zero in a field means its default (iterations 20, min_half 16, max_levels 32); NULL: all defaults.
 * Checks of order_postings, in this order: null arguments; the offsets (not starting at 0, or decreasing: DS2I_EINVAL); a doc-id
 * >= num_docs or a list that does not strictly increase (DS2I_EFORMAT, the first offender named); num_docs >= 2^32 - 2; iterations
 * > 65536 or max_levels > 32 (DS2I_EINVAL). On an error nothing is written. Sorting is spread over at most 16 host threads (threads
 * <= 0: up to 16).
 * postings_cost: the sum of LOGQ[gap] over all postings, a list's first gap being doc + 1: the size of a collection under an ideal gap
 * coder in 1/256 bits, an exact integer, so that "a better order" needs no float. Lists that do not strictly increase are DS2I_EFORMAT. */
typedef struct ds2i_order_params {
    uint32_t iterations, min_half, max_levels;
} ds2i_order_params;
int ds2i_order_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const ds2i_order_params* params,
                        int threads, ds2i_blob** doc_map, ds2i_blob** trace);
int ds2i_order_log_table(uint64_t n, uint32_t* out);
int ds2i_postings_cost(uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, uint64_t* cost);
/* test hook: the int32 a gain is clamped to before the sort and the swap see it */
int32_t ds2i_order_clamp_gain(int64_t gain);

/* The chunk directory ds2i_hip_index_open builds for one list of an opt image (inspection / test hook):
 * cmax = u32[nchunks] last doc-id per chunk, chunks = nchunks x 12 dwords (ds2i_amd/csrc/device_pef.hpp),
 * info = {n, docs_bit0, freqs_bit0, docs bit-vector byte offset in the image, freqs bit-vector byte offset} */
int ds2i_opt_list_directory(const void* opt_image, size_t bytes, uint32_t term, ds2i_blob** cmax, ds2i_blob** chunks,
                            uint64_t info[5]);
/* same for any freq_index kind (DS2I_OPT / DS2I_EF / DS2I_SINGLE / DS2I_UNIFORM) */
int ds2i_freq_list_directory(int kind, const void* image, size_t bytes, uint32_t term, ds2i_blob** cmax,
                             ds2i_blob** chunks, uint64_t info[5]);

/* block_mixed space/time optimiser (reference optimal_hybrid_index.cpp + mixed_block.hpp:119-150).
 * For every block: OptPFor with each usable b, VarInt-G8IU, interpolative -> (bytes, model time x (access + 1));
 * globally: minimise the summed time subject to summed payload bytes <= budget (lower convex hull per block +
 * one Lagrange multiplier). The time model is the MI355X kernels' instruction cost per block (defaults measured with
 * rocprofv3), the access counts come from ds2i_hip_batch_block_profile (2 per block, list by list) or NULL. */
typedef struct ds2i_hybrid ds2i_hybrid;
typedef struct ds2i_hybrid_model {
    float pfor_base, pfor_exc, pfor_exc_many, varint, interp_base, interp_node;
} ds2i_hybrid_model;
void ds2i_hybrid_default_model(ds2i_hybrid_model* m);
int ds2i_hybrid_create(uint64_t num_docs, const ds2i_hybrid_model* model /* NULL = default */, ds2i_hybrid** out);
int ds2i_hybrid_add_posting_list(ds2i_hybrid* h, uint64_t n, const uint32_t* docs, const uint32_t* freqs,
                                 const uint32_t* access /* 2 * ceil(n/128) counters or NULL */);
/* computes every block's candidates; min_space / max_space = payload bytes of the smallest / fastest index */
int ds2i_hybrid_analyse(ds2i_hybrid* h, int threads, uint64_t* min_space, uint64_t* max_space);
/* encodes the block_mixed image for the budget (payload bytes; pass UINT64_MAX for the fastest index).
 * rate = bytes spent per unit of model time saved at the optimum, type_counts = full blocks by
 * {docs pfor, docs varint, docs interpolative, freqs pfor, freqs varint, freqs interpolative} */
int ds2i_hybrid_freeze(ds2i_hybrid* h, uint64_t budget_bytes, int threads, ds2i_blob** image, double* rate,
                       uint64_t* space, double* model_time, uint64_t type_counts[6]);
/* hull of one part after analyse (either path: this one or ds2i_hip_hybrid_analyse, ds2i_hip.h): side 0 = docs,
 * 1 = freqs; points as {float time; uint16 space; uint8 type; int8 b}, by increasing space and decreasing time.
 * n receives the hull's size, at most `capacity` points are written. */
int ds2i_hybrid_hull(const ds2i_hybrid* h, uint64_t list, uint64_t block, int side, void* points, uint32_t capacity, uint32_t* n);
void ds2i_hybrid_free(ds2i_hybrid* h);

/* synthetic collection */
uint64_t ds2i_synth_list_upper_bound(const ds2i_synth_params* p, uint32_t term);
int ds2i_synth_list(const ds2i_synth_params* p, uint32_t term, uint32_t* docs, uint32_t* freqs, uint64_t capacity,
                    uint64_t* n);
int ds2i_synth_doc_sizes(const ds2i_synth_params* p, uint32_t* sizes);
/* query log: terms gets at most 11*nq entries, offsets nq+1 */
int ds2i_synth_queries(uint64_t seed, uint32_t num_terms, uint32_t nq, uint32_t* terms, uint32_t* offsets);
/* the same log with same_topic_pct percent of the multi-term queries drawn from one topic of a correlated collection */
int ds2i_synth_queries_topical(const ds2i_synth_params* p, uint64_t seed, uint32_t nq, uint32_t same_topic_pct, uint32_t* terms, uint32_t* offsets);
/* generate + encode the whole collection with `threads` host threads: index image + wand image */
int ds2i_synth_build(const ds2i_synth_params* p, int codec, int threads, ds2i_blob** index_image,
                     ds2i_blob** wand_image, uint64_t* total_postings);

/* the synthetic collection encoded by the block_mixed optimiser (lists regenerated for each pass):
 * payload budget = smallest + budget_frac * (fastest - smallest); access = 2 counters per block or NULL (uniform) */
int ds2i_synth_build_hybrid(const ds2i_synth_params* p, int threads, const ds2i_hybrid_model* model, const uint32_t* access,
                            double budget_frac, ds2i_blob** index_image, ds2i_blob** wand_image, uint64_t* total_postings,
                            uint64_t type_counts[6]);

#ifdef __cplusplus
}
#endif
#endif
