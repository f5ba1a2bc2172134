// Host-side (CPU) implementation of include/ds2i_build.h. No GPU work here.
#include <atomic>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_error.hpp"
#include "capi_hybrid.hpp"
#include "capi_partition.hpp"
#include "capi_split.hpp"
#include "host_encode.hpp"
#include "host_index.hpp"
#include "host_invert.hpp"
#include "host_pef.hpp"
#include "host_hybrid.hpp"
#include "host_merge.hpp"
#include "host_order.hpp"
#include "host_parallel.hpp"
#include "host_remap.hpp"
#include "host_shard.hpp"
#include "host_synth.hpp"

using namespace ds2i_host;

struct ds2i_builder {
    std::unique_ptr<block_index_builder> b;   // kinds 0..4
    std::unique_ptr<opt_index_builder> opt;   // kinds 5..8 (DS2I_OPT / EF / SINGLE / UNIFORM)
};
struct ds2i_wand_builder {
    std::vector<float> norm_lens, max_w;
};

extern "C" {

const uint8_t* ds2i_blob_data(const ds2i_blob* b) { return b ? b->data.data() : nullptr; }
size_t ds2i_blob_size(const ds2i_blob* b) { return b ? b->data.size() : 0; }
void ds2i_blob_free(ds2i_blob* b) { delete b; }

int ds2i_builder_create(int codec, uint64_t num_docs, ds2i_builder** out) {
    if (!out || codec < 0 || codec > LAYOUT_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_builder_create: bad argument");
    DS2I_TRY
    auto* h = new ds2i_builder;
    if (is_freq_layout(codec)) h->opt.reset(new opt_index_builder(num_docs, global_parameters(), codec));
    else h->b.reset(new block_index_builder(codec, num_docs));
    *out = h;
    return 0;
    DS2I_CATCH
}
int ds2i_builder_add_posting_list(ds2i_builder* b, uint64_t n, const uint32_t* docs, const uint32_t* freqs) {
    if (!b || !docs || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_builder_add_posting_list: null argument");
    DS2I_TRY
    if (b->opt) b->opt->add_posting_list(n, docs, freqs);
    else b->b->add_posting_list(n, docs, freqs);
    return 0;
    DS2I_CATCH
}
int ds2i_builder_freeze(ds2i_builder* b, ds2i_blob** image) {
    if (!b || !image) return ds2i_set_error(DS2I_EINVAL, "ds2i_builder_freeze: null argument");
    DS2I_TRY
    auto* blob = new ds2i_blob;
    if (b->opt) b->opt->freeze(blob->data);
    else b->b->freeze(blob->data);
    *image = blob;
    return 0;
    DS2I_CATCH
}
void ds2i_builder_free(ds2i_builder* b) { delete b; }

int ds2i_wand_create(const uint32_t* doc_sizes, uint64_t num_docs, ds2i_wand_builder** out) {
    if (!doc_sizes || !out || !num_docs) return ds2i_set_error(DS2I_EINVAL, "ds2i_wand_create: bad argument");
    DS2I_TRY
    auto* w = new ds2i_wand_builder;
    compute_norm_lens(doc_sizes, num_docs, w->norm_lens);
    *out = w;
    return 0;
    DS2I_CATCH
}
int ds2i_wand_add_list(ds2i_wand_builder* w, uint64_t n, const uint32_t* docs, const uint32_t* freqs) {
    if (!w || !docs || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_wand_add_list: null argument");
    for (uint64_t i = 0; i < n; ++i)
        if (docs[i] >= w->norm_lens.size()) return ds2i_set_error(DS2I_EINVAL, "ds2i_wand_add_list: doc id out of range");
    w->max_w.push_back(list_max_weight(w->norm_lens.data(), n, docs, freqs));
    return 0;
}
int ds2i_wand_freeze(ds2i_wand_builder* w, ds2i_blob** image) {
    if (!w || !image) return ds2i_set_error(DS2I_EINVAL, "ds2i_wand_freeze: null argument");
    DS2I_TRY
    auto* blob = new ds2i_blob;
    wand_freeze(w->norm_lens, w->max_w, blob->data);
    *image = blob;
    return 0;
    DS2I_CATCH
}
void ds2i_wand_free(ds2i_wand_builder* w) { delete w; }

int ds2i_encode_block(int codec, const uint32_t* values, uint32_t sum, uint32_t n, ds2i_blob** out) {
    if (!values || !out || n == 0 || n > BLOCK) return ds2i_set_error(DS2I_EINVAL, "ds2i_encode_block: bad argument");
    DS2I_TRY
    auto* blob = new ds2i_blob;
    block_encode(codec, values, sum, n, blob->data);
    *out = blob;
    return 0;
    DS2I_CATCH
}
// the host half of the BM25 scorer exactly as the query path uses it (query weights in plan_batch, max_term_weight in
// the wand builder); element-wise so that tests can hold it against the reference's bm25.hpp
int ds2i_bm25_query_term_weight(const uint64_t* qtf, const uint64_t* df, uint64_t num_docs, uint64_t n, float* out) {
    if (!qtf || !df || !out) return ds2i_set_error(DS2I_EINVAL, "ds2i_bm25_query_term_weight: null argument");
    for (uint64_t i = 0; i < n; ++i) out[i] = ds2i_host::bm25::query_term_weight(qtf[i], df[i], num_docs);
    return 0;
}
int ds2i_bm25_doc_term_weight(const uint64_t* freq, const float* norm_len, uint64_t n, float* out) {
    if (!freq || !norm_len || !out) return ds2i_set_error(DS2I_EINVAL, "ds2i_bm25_doc_term_weight: null argument");
    for (uint64_t i = 0; i < n; ++i) out[i] = ds2i_host::bm25::doc_term_weight(freq[i], norm_len[i]);
    return 0;
}

int ds2i_write_sequence(int seq_kind, const uint64_t* values, uint64_t n, uint64_t universe, const uint8_t params[5],
                        ds2i_blob** bits, uint64_t* nbits) {
    if (!values || !bits || !nbits || !n) return ds2i_set_error(DS2I_EINVAL, "ds2i_write_sequence: bad argument");
    DS2I_TRY
    ds2i_host::global_parameters gp;
    if (params) {
        gp.ef_log_sampling0 = params[0];
        gp.ef_log_sampling1 = params[1];
        gp.rb_log_rank1_sampling = params[2];
        gp.rb_log_sampling1 = params[3];
        gp.log_partition_size = params[4];
    }
    ds2i_host::bitvec_builder bvb;
    switch (seq_kind) {
    case DS2I_SEQ_ELIAS_FANO: ds2i_host::ef_write(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_RANKED_BITVECTOR: ds2i_host::rb_write(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_INDEXED: ds2i_host::seq_write<false>(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_STRICT: ds2i_host::seq_write<true>(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_PARTITIONED_INDEXED: ds2i_host::partitioned_write<false>(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_PARTITIONED_STRICT: ds2i_host::partitioned_write<true>(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_UNIFORM_INDEXED: ds2i_host::uniform_write<false>(bvb, values, universe, n, gp); break;
    case DS2I_SEQ_UNIFORM_STRICT: ds2i_host::uniform_write<true>(bvb, values, universe, n, gp); break;
    default: return ds2i_set_error(DS2I_EINVAL, "ds2i_write_sequence: unknown sequence kind");
    }
    auto* blob = new ds2i_blob;
    const uint8_t* w = (const uint8_t*)bvb.words().data();
    blob->data.assign(w, w + 8 * bvb.words().size());
    *nbits = bvb.size();
    *bits = blob;
    return 0;
    DS2I_CATCH
}

int ds2i_encode_vbyte(uint32_t value, ds2i_blob** out) {
    if (!out) return ds2i_set_error(DS2I_EINVAL, "ds2i_encode_vbyte: null argument");
    auto* blob = new ds2i_blob;
    vbyte_encode(value, blob->data);
    *out = blob;
    return 0;
}
int ds2i_encode_posting_list(int codec, uint32_t n, const uint32_t* docs, const uint32_t* freqs, ds2i_blob** out) {
    if (!docs || !freqs || !out || !n) return ds2i_set_error(DS2I_EINVAL, "ds2i_encode_posting_list: bad argument");
    DS2I_TRY
    auto* blob = new ds2i_blob;
    write_posting_list(codec, blob->data, n, docs, freqs);
    *out = blob;
    return 0;
    DS2I_CATCH
}

int ds2i_opt_partition(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                       ds2i_blob** docs_ends, ds2i_blob** docs_offs, ds2i_blob** freqs_ends, ds2i_blob** freqs_offs) {
    if (!list_offsets || !docs || !freqs || !docs_ends || !docs_offs || !freqs_ends || !freqs_offs)
        return ds2i_set_error(DS2I_EINVAL, "ds2i_opt_partition: null argument");
    DS2I_TRY
    const std::string fault = freq_postings_fault("ds2i_opt_partition", num_docs, nlists, list_offsets, docs, freqs);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    opt_partitions parts;
    host_opt_partitions(num_docs, nlists, list_offsets, docs, freqs, parts);
    partition_blobs(parts, docs_ends, docs_offs, freqs_ends, freqs_offs);
    return 0;
    DS2I_CATCH
}

int ds2i_check_doc_map(const uint32_t* doc_map, uint64_t num_docs) {
    if (!doc_map && num_docs) return ds2i_set_error(DS2I_EINVAL, "ds2i_check_doc_map: null argument");
    DS2I_TRY
    const std::string fault = doc_map_fault(doc_map, num_docs);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, ("ds2i_check_doc_map: " + fault).c_str());
    return 0;
    DS2I_CATCH
}

int ds2i_remap_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, uint32_t* docs, uint32_t* freqs, const uint32_t* doc_map,
                        int threads) {
    if (!list_offsets || !docs || !freqs || !doc_map) return ds2i_set_error(DS2I_EINVAL, "ds2i_remap_postings: null argument");
    if (list_offsets[0] != 0) return ds2i_set_error(DS2I_EINVAL, "ds2i_remap_postings: list_offsets must start at 0");
    for (uint64_t t = 0; t < nlists; ++t)
        if (list_offsets[t + 1] < list_offsets[t]) return ds2i_set_error(DS2I_EINVAL, "ds2i_remap_postings: list_offsets decrease");
    const int rc = ds2i_check_doc_map(doc_map, num_docs);
    if (rc != 0) return rc;
    DS2I_TRY
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    remap_postings(num_docs, nlists, list_offsets, docs, freqs, doc_map, (unsigned)threads);
    return 0;
    DS2I_CATCH
}

int ds2i_remap_wand(const void* wand_image, size_t bytes, const uint32_t* doc_map, uint64_t num_docs, ds2i_blob** out) {
    if (!wand_image || !doc_map || !out) return ds2i_set_error(DS2I_EINVAL, "ds2i_remap_wand: null argument");
    DS2I_TRY
    wand_view w;
    w.parse(wand_image, bytes);
    if (w.num_docs != num_docs) return ds2i_set_error(DS2I_EINVAL, "ds2i_remap_wand: the map's length is not the wand data's number of documents");
    const int rc = ds2i_check_doc_map(doc_map, num_docs);
    if (rc != 0) return rc;
    std::unique_ptr<ds2i_blob> blob(new ds2i_blob);
    remap_wand(w, doc_map, blob->data);
    *out = blob.release();
    return 0;
    DS2I_CATCH
}

int ds2i_split_wand(const void* wand_image, size_t bytes, const uint32_t* doc_map, uint64_t ndocs, const uint32_t* term_map, uint64_t nterms,
                    ds2i_blob** out) {
    if (!wand_image || !out || (!doc_map && ndocs) || (!term_map && nterms)) return ds2i_set_error(DS2I_EINVAL, "ds2i_split_wand: null argument");
    DS2I_TRY
    wand_view w;
    w.parse(wand_image, bytes);
    const std::string fault = split_wand_fault("ds2i_split_wand", w, doc_map, ndocs, term_map, nterms);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    std::unique_ptr<ds2i_blob> blob(new ds2i_blob);
    split_wand(w, doc_map, ndocs, term_map, nterms, blob->data);
    *out = blob.release();
    return 0;
    DS2I_CATCH
}

int ds2i_wand_arrays(const void* wand_image, size_t bytes, ds2i_blob** norm_lens, ds2i_blob** max_term_weight) {
    if (!wand_image || (!norm_lens && !max_term_weight)) return ds2i_set_error(DS2I_EINVAL, "ds2i_wand_arrays: null argument");
    DS2I_TRY
    wand_view w;
    w.parse(wand_image, bytes);
    std::unique_ptr<ds2i_blob> a(new ds2i_blob), b(new ds2i_blob);
    a->data.assign(w.norm_lens, w.norm_lens + 4 * w.num_docs);
    b->data.assign(w.max_term_weight, w.max_term_weight + 4 * w.num_terms);
    if (norm_lens) *norm_lens = a.release();
    if (max_term_weight) *max_term_weight = b.release();
    return 0;
    DS2I_CATCH
}

int ds2i_merge_topk(const ds2i_topk_rows* rows, uint32_t nrows, uint32_t nq, uint32_t k, float* out_scores, uint32_t* out_docs, uint32_t* out_lens,
                    int threads) {
    DS2I_TRY
    const std::string fault = merge_topk_fault("ds2i_merge_topk", rows, nrows, nq, k, nq && (!out_scores || !out_docs || !out_lens));
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (!nq) return 0;
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = std::min(threads, 16);
    merge_topk(rows, nrows, nq, k, out_scores, out_docs, out_lens, (unsigned)threads);
    return 0;
    DS2I_CATCH
}

int ds2i_merge_postings(const ds2i_merge_postings_source* src, uint32_t nsrc, uint64_t nlists, int threads, uint64_t* num_docs, uint64_t* out_nlists,
                        ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs) {
    if (!num_docs || !out_nlists || !list_offsets || !docs || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_merge_postings: null argument");
    DS2I_TRY
    std::vector<merge_shape> shapes;
    merge_plan plan;
    std::string fault = merge_csr_fault("ds2i_merge_postings", src, nsrc, shapes);
    if (fault.empty()) fault = merge_plan_fault("ds2i_merge_postings", shapes.data(), nsrc, nlists, plan);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = std::min(threads, 16);
    std::vector<const uint32_t*> d(nsrc), f(nsrc);
    for (uint32_t s = 0; s < nsrc; ++s) {
        d[s] = src[s].docs;
        f[s] = src[s].freqs;
    }
    const uint64_t total = plan.offs[plan.nlists];
    std::unique_ptr<ds2i_blob> bo(new ds2i_blob), bd(new ds2i_blob), bf(new ds2i_blob);
    bo->data.resize(8 * (plan.nlists + 1));
    std::memcpy(bo->data.data(), plan.offs.data(), 8 * (plan.nlists + 1));
    bd->data.resize(4 * total);
    bf->data.resize(4 * total);
    merge_postings(shapes.data(), d.data(), f.data(), nsrc, plan, (uint32_t*)bd->data.data(), (uint32_t*)bf->data.data(), (unsigned)threads);
    *num_docs = plan.num_docs;
    *out_nlists = plan.nlists;
    *list_offsets = bo.release();
    *docs = bd.release();
    *freqs = bf.release();
    return 0;
    DS2I_CATCH
}

int ds2i_split_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                        const uint32_t* shard_of, uint32_t nshards, int threads, ds2i_split_shard** shards) {
    static const char* const who = "ds2i_split_postings";
    if (!list_offsets || !docs || !freqs || (!shard_of && num_docs) || !shards) return ds2i_set_error(DS2I_EINVAL, "ds2i_split_postings: null argument");
    DS2I_TRY
    std::string fault = split_csr_fault(who, nlists, list_offsets);
    if (fault.empty()) fault = split_assign_fault(who, num_docs, nlists, shard_of, nshards);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = std::min(threads, 16);
    std::vector<split_shard> out;
    split_postings(num_docs, nlists, list_offsets, docs, freqs, shard_of, nshards, (unsigned)threads, out);
    SplitShards arr = new_split_shards(nshards);
    for (uint32_t s = 0; s < nshards; ++s) {
        fill_split_shard(arr.get()[s], out[s], true);
        out[s] = split_shard(); // (a shard's vectors go as soon as its blobs stand)
    }
    *shards = arr.release();
    return 0;
    DS2I_CATCH
}

void ds2i_split_free(ds2i_split_shard* shards, uint32_t nshards) {
    if (!shards) return;
    for (uint32_t s = 0; s < nshards; ++s)
        for (ds2i_blob* b : {shards[s].doc_map, shards[s].term_map, shards[s].list_offsets, shards[s].docs, shards[s].freqs, shards[s].image}) delete b;
    delete[] shards;
}

int ds2i_invert_documents(uint64_t num_docs, const uint64_t* doc_offsets, const uint32_t* tokens, uint64_t nterms, int threads, ds2i_blob** list_offsets,
                          ds2i_blob** docs, ds2i_blob** freqs, ds2i_blob** doc_sizes) {
    static const char* const who = "ds2i_invert_documents";
    if (!doc_offsets || !tokens || !list_offsets || !docs || !freqs || !doc_sizes) return ds2i_set_error(DS2I_EINVAL, "ds2i_invert_documents: null argument");
    DS2I_TRY
    const std::string fault = invert_shape_fault(who, num_docs, nterms, doc_offsets);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = std::min(threads, 16);
    csr_matrix lists;
    std::vector<uint32_t> sizes;
    invert_documents(who, num_docs, doc_offsets, tokens, nterms, (unsigned)threads, lists, sizes);
    std::unique_ptr<ds2i_blob> bo(ds2i_blob_of(lists.offs)), bd(ds2i_blob_of(lists.ids)), bf(ds2i_blob_of(lists.vals)), bs(ds2i_blob_of(sizes));
    *list_offsets = bo.release();
    *docs = bd.release();
    *freqs = bf.release();
    *doc_sizes = bs.release();
    return 0;
    DS2I_CATCH
}

int ds2i_transpose_postings(uint64_t nrows, uint64_t ncols, const uint64_t* row_offsets, const uint32_t* cols, const uint32_t* vals, int threads,
                            ds2i_blob** col_offsets, ds2i_blob** rows, ds2i_blob** out_vals) {
    static const char* const who = "ds2i_transpose_postings";
    if (!row_offsets || !cols || !vals || !col_offsets || !rows || !out_vals) return ds2i_set_error(DS2I_EINVAL, "ds2i_transpose_postings: null argument");
    DS2I_TRY
    const std::string fault = transpose_shape_fault(who, nrows, ncols, row_offsets);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = std::min(threads, 16);
    check_columns(who, nrows, ncols, row_offsets, cols, (unsigned)threads);
    csr_matrix t;
    transpose_csr(nrows, ncols, row_offsets, cols, vals, (unsigned)threads, t);
    std::unique_ptr<ds2i_blob> bo(ds2i_blob_of(t.offs)), br(ds2i_blob_of(t.ids)), bv(ds2i_blob_of(t.vals));
    *col_offsets = bo.release();
    *rows = br.release();
    *out_vals = bv.release();
    return 0;
    DS2I_CATCH
}

int ds2i_order_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const ds2i_order_params* params,
                        int threads, ds2i_blob** doc_map, ds2i_blob** trace) {
    static const char* const who = "ds2i_order_postings";
    if (!list_offsets || !docs || !doc_map || !trace) return ds2i_set_error(DS2I_EINVAL, "ds2i_order_postings: null argument");
    DS2I_TRY
    std::string fault = order_offsets_fault(who, nlists, list_offsets);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    fault = order_docs_fault(who, num_docs, nlists, list_offsets, docs);
    if (!fault.empty()) return ds2i_set_error(DS2I_EFORMAT, fault.c_str());
    order_params prm;
    fault = order_num_docs_fault(who, num_docs);
    if (fault.empty()) fault = order_params_fault(who, params ? params->iterations : 0, params ? params->min_half : 0, params ? params->max_levels : 0, prm);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (threads <= 0) threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    threads = std::min(threads, 16);
    std::vector<uint32_t> map;
    std::vector<uint64_t> tr;
    order_postings(num_docs, nlists, list_offsets, docs, prm, (unsigned)threads, map, tr);
    std::unique_ptr<ds2i_blob> bm(ds2i_blob_of(map)), bt(ds2i_blob_of(tr));
    *doc_map = bm.release();
    *trace = bt.release();
    return 0;
    DS2I_CATCH
}

int ds2i_order_log_table(uint64_t n, uint32_t* out) {
    if (!out) return ds2i_set_error(DS2I_EINVAL, "ds2i_order_log_table: null argument");
    order_log_table(n, out);
    return 0;
}

int ds2i_postings_cost(uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, uint64_t* cost) {
    static const char* const who = "ds2i_postings_cost";
    if (!list_offsets || !docs || !cost) return ds2i_set_error(DS2I_EINVAL, "ds2i_postings_cost: null argument");
    DS2I_TRY
    std::string fault = order_offsets_fault(who, nlists, list_offsets);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    fault = order_docs_fault(who, 1ull << 32, nlists, list_offsets, docs);
    if (!fault.empty()) return ds2i_set_error(DS2I_EFORMAT, fault.c_str());
    *cost = postings_cost(nlists, list_offsets, docs);
    return 0;
    DS2I_CATCH
}

int32_t ds2i_order_clamp_gain(int64_t gain) { return order_clamp_gain(gain); }

int ds2i_opt_list_directory(const void* opt_image, size_t bytes, uint32_t term, ds2i_blob** cmax, ds2i_blob** chunks,
                            uint64_t info[5]) {
    return ds2i_freq_list_directory(LAYOUT_OPT, opt_image, bytes, term, cmax, chunks, info);
}
int ds2i_freq_list_directory(int kind, const void* opt_image, size_t bytes, uint32_t term, ds2i_blob** cmax,
                             ds2i_blob** chunks, uint64_t info[5]) {
    if (!opt_image || !cmax || !chunks || !info || !is_freq_layout(kind))
        return ds2i_set_error(DS2I_EINVAL, "ds2i_freq_list_directory: bad argument");
    DS2I_TRY
    opt_index_view v;
    v.layout = kind;
    v.parse(opt_image, bytes);
    if (term >= v.size) return ds2i_set_error(DS2I_ETERM, "term id out of range");
    pef_list_dir dir;
    v.build_dir(term, dir);
    auto* bc = new ds2i_blob;
    auto* bk = new ds2i_blob;
    const uint8_t* p = (const uint8_t*)dir.cmax.data();
    bc->data.assign(p, p + 4 * dir.cmax.size());
    p = (const uint8_t*)dir.chunks.data();
    bk->data.assign(p, p + sizeof(pef_chunk) * dir.chunks.size());
    *cmax = bc;
    *chunks = bk;
    info[0] = dir.n;
    info[1] = dir.docs_bit0;
    info[2] = dir.freqs_bit0;
    info[3] = (uint64_t)(v.docs_bits.bytes - (const uint8_t*)opt_image);
    info[4] = (uint64_t)(v.freqs_bits.bytes - (const uint8_t*)opt_image);
    return 0;
    DS2I_CATCH
}

uint64_t ds2i_synth_list_upper_bound(const ds2i_synth_params* p, uint32_t term) {
    (void)term;
    return p ? p->num_docs : 0;
}
int ds2i_synth_list(const ds2i_synth_params* p, uint32_t term, uint32_t* docs, uint32_t* freqs, uint64_t capacity,
                    uint64_t* n) {
    if (!p || !docs || !freqs || !n) return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_list: null argument");
    DS2I_TRY
    std::vector<uint32_t> d, f;
    uint64_t len = synth_list(to_params(p), term, d, f);
    *n = len;
    if (len > capacity) return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_list: capacity too small");
    std::memcpy(docs, d.data(), 4 * len);
    std::memcpy(freqs, f.data(), 4 * len);
    return 0;
    DS2I_CATCH
}
int ds2i_synth_doc_sizes(const ds2i_synth_params* p, uint32_t* sizes) {
    if (!p || !sizes) return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_doc_sizes: null argument");
    DS2I_TRY
    std::vector<uint32_t> s;
    synth_doc_sizes(to_params(p), s);
    std::memcpy(sizes, s.data(), 4 * s.size());
    return 0;
    DS2I_CATCH
}
int ds2i_synth_queries(uint64_t seed, uint32_t num_terms, uint32_t nq, uint32_t* terms, uint32_t* offsets) {
    if (!terms || !offsets || !num_terms) return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_queries: bad argument");
    DS2I_TRY
    std::vector<uint32_t> t, o;
    synth_queries(seed, num_terms, nq, t, o);
    std::memcpy(terms, t.data(), 4 * t.size());
    std::memcpy(offsets, o.data(), 4 * o.size());
    return 0;
    DS2I_CATCH
}

int ds2i_synth_queries_topical(const ds2i_synth_params* pp, uint64_t seed, uint32_t nq, uint32_t same_topic_pct, uint32_t* terms, uint32_t* offsets) {
    if (!pp || !terms || !offsets || !pp->num_terms) return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_queries_topical: bad argument");
    DS2I_TRY
    std::vector<uint32_t> t, o;
    synth_queries_topical(to_params(pp), seed, nq, same_topic_pct, t, o);
    std::memcpy(terms, t.data(), 4 * t.size());
    std::memcpy(offsets, o.data(), 4 * o.size());
    return 0;
    DS2I_CATCH
}

int ds2i_synth_build(const ds2i_synth_params* pp, int codec, int threads, ds2i_blob** index_image,
                     ds2i_blob** wand_image, uint64_t* total_postings) {
    if (!pp || !index_image || codec < 0 || codec > LAYOUT_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_build: bad argument");
    const bool freq_layout = is_freq_layout(codec);
    DS2I_TRY
    const synth_params p = to_params(pp);
    if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
    std::vector<uint32_t> sizes;
    synth_doc_sizes(p, sizes);
    std::vector<float> norm_lens;
    compute_norm_lens(sizes.data(), p.num_docs, norm_lens);
    sizes.clear();
    sizes.shrink_to_fit();
    const uint32_t V = p.num_terms;
    std::vector<bytes_t> enc(V);
    std::vector<bitvec_builder> enc_docs(freq_layout ? V : 0), enc_freqs(freq_layout ? V : 0);
    std::vector<float> max_w(V);
    std::atomic<uint64_t> postings(0);
    std::vector<std::vector<uint32_t>> d(threads), f(threads); // every worker's list
    parallel_for(V, (unsigned)threads, [&](uint64_t t, unsigned w) {
        const uint64_t n = synth_list(p, (uint32_t)t, d[w], f[w]);
        if (freq_layout) opt_index_builder::encode_list(p.num_docs, global_parameters(), n, d[w].data(), f[w].data(), enc_docs[t], enc_freqs[t], codec);
        else write_posting_list(codec, enc[t], (uint32_t)n, d[w].data(), f[w].data());
        max_w[t] = list_max_weight(norm_lens.data(), n, d[w].data(), f[w].data());
        postings += n;
    });
    auto* ib = new ds2i_blob;
    if (freq_layout) {
        opt_index_builder builder(p.num_docs, global_parameters(), codec);
        for (uint32_t t = 0; t < V; ++t) {
            builder.add_encoded(enc_docs[t], enc_freqs[t]);
            enc_docs[t] = bitvec_builder();
            enc_freqs[t] = bitvec_builder();
        }
        builder.freeze(ib->data);
    } else {
        block_index_builder builder(codec, p.num_docs);
        for (uint32_t t = 0; t < V; ++t) {
            builder.add_encoded_list(enc[t].data(), enc[t].size());
            bytes_t().swap(enc[t]);
        }
        builder.freeze(ib->data);
    }
    *index_image = ib;
    if (wand_image) {
        auto* wb = new ds2i_blob;
        wand_freeze(norm_lens, max_w, wb->data);
        *wand_image = wb;
    }
    if (total_postings) *total_postings = postings;
    return 0;
    DS2I_CATCH
}


// ---------------------------------------------------------------- block_mixed optimiser (host_hybrid.hpp)
void ds2i_hybrid_default_model(ds2i_hybrid_model* m) {
    if (m) *m = from_model(hybrid_model());
}
int ds2i_hybrid_create(uint64_t num_docs, const ds2i_hybrid_model* model, ds2i_hybrid** out) {
    if (!out) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_create: null argument");
    DS2I_TRY
    auto* h = new ds2i_hybrid;
    h->b.reset(new hybrid_index_builder(num_docs, to_model(model)));
    *out = h;
    return 0;
    DS2I_CATCH
}
int ds2i_hybrid_add_posting_list(ds2i_hybrid* h, uint64_t n, const uint32_t* docs, const uint32_t* freqs, const uint32_t* access) {
    if (!h || !docs || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_add_posting_list: null argument");
    DS2I_TRY
    h->b->add_posting_list(n, docs, freqs, access);
    return 0;
    DS2I_CATCH
}
int ds2i_hybrid_analyse(ds2i_hybrid* h, int threads, uint64_t* min_space, uint64_t* max_space) {
    if (!h) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_analyse: null argument");
    DS2I_TRY
    if (!h->b->analysed()) h->b->analyse(threads);
    if (min_space) *min_space = h->b->min_space();
    if (max_space) *max_space = h->b->max_space();
    return 0;
    DS2I_CATCH
}
int ds2i_hybrid_freeze(ds2i_hybrid* h, uint64_t budget_bytes, int threads, ds2i_blob** image, double* rate, uint64_t* space,
                       double* model_time, uint64_t type_counts[6]) {
    if (!h || !image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_freeze: null argument");
    DS2I_TRY
    if (!h->b->analysed()) h->b->analyse(threads);
    if (budget_bytes < h->b->min_space()) return ds2i_set_error(DS2I_EINVAL, "budget below the smallest possible index");
    const double r = h->b->solve(budget_bytes);
    uint64_t s = 0;
    double t = 0;
    h->b->evaluate(r, s, t);
    auto* blob = new ds2i_blob;
    h->b->freeze(r, threads, blob->data, type_counts);
    *image = blob;
    if (rate) *rate = r;
    if (space) *space = s;
    if (model_time) *model_time = t;
    return 0;
    DS2I_CATCH
}
int ds2i_hybrid_hull(const ds2i_hybrid* h, uint64_t list, uint64_t block, int side, void* points, uint32_t capacity, uint32_t* n) {
    if (!h || !n || (!points && capacity)) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_hull: null argument");
    if (!h->b->analysed()) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_hull: the builder is not analysed");
    static_assert(sizeof(hybrid_point) == 8, "hybrid_point is the published {float, uint16, uint8, int8}");
    uint32_t cnt = 0;
    const hybrid_point* p = h->b->hull(list, block, side, cnt);
    if (!p) return ds2i_set_error(DS2I_EINVAL, "ds2i_hybrid_hull: no such part");
    *n = cnt;
    if (points && capacity) std::memcpy(points, p, sizeof(hybrid_point) * std::min(cnt, capacity));
    return 0;
}
void ds2i_hybrid_free(ds2i_hybrid* h) { delete h; }

// The synthetic collection through the optimiser: lists are regenerated (pure functions of seed and term) for the
// analysis pass and again for the encoding pass, so a GOV2- / ClueWeb-scale collection never sits in memory raw.
// budget = min_space + budget_frac * (max_space - min_space).
int ds2i_synth_build_hybrid(const ds2i_synth_params* pp, int threads, const ds2i_hybrid_model* model, const uint32_t* access,
                            double budget_frac, ds2i_blob** index_image, ds2i_blob** wand_image, uint64_t* total_postings,
                            uint64_t type_counts[6]) {
    if (!pp || !index_image || !(budget_frac >= 0.0 && budget_frac <= 1.0))
        return ds2i_set_error(DS2I_EINVAL, "ds2i_synth_build_hybrid: bad argument");
    DS2I_TRY
    const synth_params p = to_params(pp);
    if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
    const uint32_t V = p.num_terms;
    std::vector<uint32_t> sizes;
    synth_doc_sizes(p, sizes);
    std::vector<float> norm_lens;
    compute_norm_lens(sizes.data(), p.num_docs, norm_lens);
    std::vector<uint32_t>().swap(sizes);
    // pass 0: list lengths (block numbering of `access`), max term weights
    std::vector<float> max_w(V, 0.f);
    std::vector<uint64_t> len(V, 0);
    {
        std::vector<std::vector<uint32_t>> d(threads), f(threads); // every worker's list
        parallel_for(V, (unsigned)threads, [&](uint64_t t, unsigned w) {
            len[t] = synth_list(p, (uint32_t)t, d[w], f[w]);
            max_w[t] = list_max_weight(norm_lens.data(), len[t], d[w].data(), f[w].data());
        });
    }
    hybrid_index_builder hb(p.num_docs, to_model(model));
    uint64_t base = 0, postings = 0;
    for (uint32_t t = 0; t < V; ++t) {
        const uint64_t blocks = ceil_div(len[t], (uint64_t)BLOCK);
        hb.add_virtual_list(access ? access + 2 * base : nullptr, blocks);
        base += blocks;
        postings += len[t];
    }
    hb.set_provider([&](size_t t, std::vector<uint32_t>& d, std::vector<uint32_t>& f) {
        const uint64_t n = synth_list(p, (uint32_t)t, d, f);
        d.resize(n);
        f.resize(n);
    });
    hb.analyse(threads);
    const uint64_t lo = hb.min_space(), hi = hb.max_space();
    const uint64_t budget = lo + (uint64_t)(budget_frac * double(hi - lo));
    const double rate = hb.solve(budget);
    auto* ib = new ds2i_blob;
    hb.freeze(rate, threads, ib->data, type_counts);
    *index_image = ib;
    if (wand_image) {
        auto* wb = new ds2i_blob;
        wand_freeze(norm_lens, max_w, wb->data);
        *wand_image = wb;
    }
    if (total_postings) *total_postings = postings;
    return 0;
    DS2I_CATCH
}

} // extern "C"
