// Host side of querying document shards as one index (include/ds2i_hip.h: ds2i_hip_merge_topk, ds2i_hip_shard_set_*): the argument
// checks, all made on the host (host_shard.hpp, the host parse of the images) before a device is looked for; the merge of top-k rows on
// the device (shard_kernels.hip: rows and maps up, one kernel, the result down); and the shard set -- every shard an index of its own on
// its own device with the collection's BM25 statistics (ds2i_hip_index_set_collection_stats) and a pipeline of its own, the queries
// translated per shard on the host, the batches submitted together and collected, the rows brought up to the merge device and merged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_util.hpp"
#include "host_shard.hpp"
#include "launchers.hpp"

namespace {

using namespace ds2i_dev;

// the limits are stated three times -- the C header, the host twin's header (no HIP, no C ABI) and the kernels' argument blocks
static_assert(ds2i_host::SHARD_MAX_ROWS == DS2I_HIP_MAX_SHARDS && MERGE_TOPK_MAX_ROWS == DS2I_HIP_MAX_SHARDS, "one limit on the row sets of a merge");
static_assert(ds2i_host::SHARD_MAX_K == DS2I_HIP_MAX_K_LONG && MERGE_TOPK_MAX_K == DS2I_HIP_MAX_K_LONG, "one limit on k");
static_assert(DS2I_HIP_MAX_SHARDS <= 64, "MergeTopkArgs::unsorted holds one bit per row set");

// The device side of a merge on one device: grow-only buffers for the row sets, the maps and the result. A shard set keeps one for its
// life with its doc maps resident; ds2i_hip_merge_topk makes one per call.
struct MergeDevice {
    int device = 0, cus = 1;
    struct Set {
        DevBuf scores, docs, lens, map;
        uint64_t map_len = 0;
        bool has_map = false, increasing = true;
    };
    std::vector<std::unique_ptr<Set>> sets;
    DevBuf rows, out_scores, out_docs, out_lens;

    int nomem(const char* who) const {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": the rows, the doc maps and the result do not fit on the device").c_str());
    }
    int open(const char* who, int device_, uint32_t nsets) {
        device = device_;
        HIP_OK(hipSetDevice(device));
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        sets.clear();
        for (uint32_t r = 0; r < nsets; ++r) sets.emplace_back(new Set);
        return DS2I_OK;
    }
    // the doc map of row set r (null: the ids are the collection's), copied up
    int set_map(const char* who, uint32_t r, const uint32_t* doc_map, uint64_t map_len) {
        Set& s = *sets[r];
        s.has_map = doc_map != nullptr;
        s.map_len = doc_map ? map_len : 0;
        s.increasing = !doc_map || ds2i_host::map_increases(doc_map, map_len);
        if (!doc_map) return DS2I_OK;
        HIP_OK(hipSetDevice(device));
        if (s.map.reserve(4 * std::max<uint64_t>(map_len, 1)) != hipSuccess) return nomem(who);
        if (map_len) HIP_OK(hipMemcpy(s.map.p, doc_map, 4 * map_len, hipMemcpyHostToDevice));
        return DS2I_OK;
    }
    // rows[r] (host pointers; doc_map / map_len are not read: set_map's hold) merged; the outputs are host pointers
    int run(const char* who, const ds2i_topk_rows* host_rows, uint32_t nrows, uint32_t nq, uint32_t k, float* out_s, uint32_t* out_d,
            uint32_t* out_l, double& ms) {
        HIP_OK(hipSetDevice(device));
        const size_t cells = 4 * (size_t)nq * k;
        std::vector<TopkRowSet> dev_rows(nrows);
        MergeTopkArgs a{};
        for (uint32_t r = 0; r < nrows; ++r) {
            Set& s = *sets[r];
            if (s.scores.reserve(cells) != hipSuccess || s.docs.reserve(cells) != hipSuccess || s.lens.reserve(4 * (size_t)nq) != hipSuccess)
                return nomem(who);
            HIP_OK(hipMemcpy(s.scores.p, host_rows[r].scores, cells, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(s.docs.p, host_rows[r].docs, cells, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(s.lens.p, host_rows[r].lens, 4 * (size_t)nq, hipMemcpyHostToDevice));
            dev_rows[r] = TopkRowSet{(const float*)s.scores.p, (const uint32_t*)s.docs.p, (const uint32_t*)s.lens.p,
                                     s.has_map ? (const uint32_t*)s.map.p : nullptr, s.map_len};
            if (!s.increasing) a.unsorted |= 1ull << r;
        }
        if (rows.reserve(sizeof(TopkRowSet) * nrows) != hipSuccess || out_scores.reserve(cells) != hipSuccess ||
            out_docs.reserve(cells) != hipSuccess || out_lens.reserve(4 * (size_t)nq) != hipSuccess)
            return nomem(who);
        HIP_OK(hipMemcpy(rows.p, dev_rows.data(), sizeof(TopkRowSet) * nrows, hipMemcpyHostToDevice));
        a.rows = (const TopkRowSet*)rows.p;
        a.nrows = nrows;
        a.nq = nq;
        a.k = k;
        a.pow2 = merge_topk_pow2(k);
        a.out_scores = (float*)out_scores.p;
        a.out_docs = (uint32_t*)out_docs.p;
        a.out_lens = (uint32_t*)out_lens.p;
        hipStream_t stream = nullptr;
        HIP_OK(timed_span(stream, ms, [&] { return ds2i_launch_merge_topk(a, merge_topk_grid(nq, cus, k), stream); }));
        HIP_OK(hipMemcpy(out_s, out_scores.p, cells, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out_d, out_docs.p, cells, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out_l, out_lens.p, 4 * (size_t)nq, hipMemcpyDeviceToHost));
        return DS2I_OK;
    }
};

struct PipelineCloser {
    void operator()(ds2i_hip_pipeline* p) const { ds2i_hip_pipeline_destroy(p); }
};

// one opened shard of a set, with the buffers its share of a batch goes through
struct Shard {
    uint32_t source = 0; // its number among the sources
    int device = 0;
    IndexHandle idx;
    std::unique_ptr<ds2i_hip_pipeline, PipelineCloser> pipe;
    std::vector<uint32_t> term_map;
    std::vector<uint32_t> terms, offs, docs, lens;
    std::vector<uint64_t> count;
    std::vector<float> topk;
    uint64_t ticket = 0;
    bool in_flight = false;
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

struct ds2i_hip_shard_set {
    uint64_t collection_docs = 0, collection_terms = 0;
    uint32_t nsources = 0;
    std::vector<std::unique_ptr<Shard>> shards; // the opened ones, in source order
    MergeDevice merge;
};

extern "C" {

int ds2i_hip_merge_topk(int device, const ds2i_topk_rows* rows, uint32_t nrows, uint32_t nq, uint32_t k, float* out_scores, uint32_t* out_docs,
                        uint32_t* out_lens, double* device_ms) {
    static const char* const who = "ds2i_hip_merge_topk";
    DS2I_TRY
    const std::string fault = ds2i_host::merge_topk_fault(who, rows, nrows, nq, k, nq && (!out_scores || !out_docs || !out_lens));
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    if (!nq) {
        if (device_ms) *device_ms = 0.0;
        return DS2I_OK;
    }
    int rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    MergeDevice m;
    rc = m.open(who, device, nrows);
    for (uint32_t r = 0; r < nrows && rc == DS2I_OK; ++r) rc = m.set_map(who, r, rows[r].doc_map, rows[r].map_len);
    double ms = 0.0;
    if (rc == DS2I_OK) rc = m.run(who, rows, nrows, nq, k, out_scores, out_docs, out_lens, ms);
    if (rc == DS2I_OK && device_ms) *device_ms = ms;
    return rc;
    DS2I_CATCH
}

int ds2i_hip_shard_set_open(const ds2i_shard_source* src, uint32_t nshards, uint64_t collection_docs, uint64_t collection_terms,
                            uint64_t stats_num_docs, const uint32_t* stats_df, ds2i_hip_shard_set** out) {
    static const std::string who = "ds2i_hip_shard_set_open: ";
    if (!src || !out) return ds2i_set_error(DS2I_EINVAL, (who + "null argument").c_str());
    for (uint32_t s = 0; s < nshards && s < DS2I_HIP_MAX_SHARDS; ++s)
        if (!src[s].image || (!src[s].doc_map && src[s].map_len) || (!src[s].term_map && src[s].terms_len))
            return ds2i_set_error(DS2I_EINVAL, (who + "null argument").c_str());
    if (nshards == 0 || nshards > DS2I_HIP_MAX_SHARDS)
        return ds2i_set_error(DS2I_EINVAL, (who + std::to_string(nshards) + " shards: a set holds 1 to " + std::to_string(DS2I_HIP_MAX_SHARDS)).c_str());
    for (uint32_t s = 0; s < nshards; ++s)
        if (src[s].kind < DS2I_BLOCK_OPTPFOR || src[s].kind > DS2I_UNIFORM)
            return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": unknown index kind").c_str());
    DS2I_TRY
    std::vector<uint64_t> ndocs(nshards), nlists(nshards);
    std::vector<std::vector<uint32_t>> lengths(nshards);
    for (uint32_t s = 0; s < nshards; ++s) {
        const int rc = ds2i_parse_image(src[s].kind, src[s].image, src[s].bytes, ndocs[s], nlists[s], &lengths[s]);
        if (rc != DS2I_OK) return rc;
    }
    for (uint32_t s = 0; s < nshards; ++s) {
        if (src[s].map_len != ndocs[s])
            return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": doc_map holds " + std::to_string(src[s].map_len) +
                                                " documents, the index " + std::to_string(ndocs[s])).c_str());
        if (src[s].terms_len != nlists[s])
            return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": term_map holds " + std::to_string(src[s].terms_len) +
                                                " terms, the index " + std::to_string(nlists[s])).c_str());
    }
    for (uint32_t s = 0; s < nshards; ++s)
        for (uint64_t j = 0; j < nlists[s]; ++j) {
            const uint32_t t = src[s].term_map[j];
            if (t >= collection_terms)
                return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": term_map[" + std::to_string(j) + "] = " + std::to_string(t) +
                                                    " lies outside the " + std::to_string(collection_terms) + " terms of the collection").c_str());
            if (j && t <= src[s].term_map[j - 1])
                return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": term_map does not increase at entry " + std::to_string(j)).c_str());
        }
    {
        std::vector<uint64_t> taken((collection_docs + 63) / 64, 0);
        for (uint32_t s = 0; s < nshards; ++s)
            for (uint64_t i = 0; i < ndocs[s]; ++i) {
                const uint64_t g = src[s].doc_map[i];
                if (g >= collection_docs)
                    return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": document " + std::to_string(i) + " maps to " + std::to_string(g) +
                                                        ", outside the " + std::to_string(collection_docs) + " documents of the collection").c_str());
                if (taken[g >> 6] >> (g & 63) & 1)
                    return ds2i_set_error(DS2I_EINVAL, (who + "shard " + std::to_string(s) + ": document " + std::to_string(i) + " maps to " + std::to_string(g) +
                                                        ", which an earlier document took").c_str());
                taken[g >> 6] |= 1ull << (g & 63);
            }
    }
    // the statistics: the defaults are the sums over the shards
    uint64_t num_docs = stats_num_docs;
    if (!num_docs)
        for (uint32_t s = 0; s < nshards; ++s) num_docs += ndocs[s];
    std::vector<uint64_t> df_sum(collection_terms, 0);
    for (uint32_t s = 0; s < nshards; ++s)
        for (uint64_t j = 0; j < nlists[s]; ++j) df_sum[src[s].term_map[j]] += lengths[s][j];
    for (uint64_t t = 0; t < collection_terms; ++t) {
        const uint64_t df = stats_df ? stats_df[t] : df_sum[t];
        if (df < df_sum[t] || df > num_docs)
            return ds2i_set_error(DS2I_EINVAL, (who + "term " + std::to_string(t) + ": df " + std::to_string(df) + " lies outside the sum of its shard lists " +
                                                std::to_string(df_sum[t]) + " .. the collection's " + std::to_string(num_docs) + " documents").c_str());
    }
    for (uint32_t s = 0; s < nshards; ++s)
        if (num_docs < ndocs[s])
            return ds2i_set_error(DS2I_EINVAL, (who + "a collection of " + std::to_string(num_docs) + " documents is smaller than shard " +
                                                std::to_string(s) + "'s " + std::to_string(ndocs[s])).c_str());
    // the devices
    std::unique_ptr<ds2i_hip_shard_set> set(new ds2i_hip_shard_set);
    set->collection_docs = collection_docs;
    set->collection_terms = collection_terms;
    set->nsources = nshards;
    for (uint32_t s = 0; s < nshards; ++s) {
        if (!ndocs[s] || !nlists[s]) continue; // nothing to answer with
        int rc = check_device("ds2i_hip_shard_set_open", src[s].device);
        if (rc != DS2I_OK) return rc;
        std::unique_ptr<Shard> sh(new Shard);
        sh->source = s;
        sh->device = src[s].device;
        ds2i_hip_index* raw = nullptr;
        rc = ds2i_hip_index_open(src[s].device, src[s].kind, src[s].image, src[s].bytes, src[s].wand_image, src[s].wand_image ? src[s].wand_bytes : 0, &raw);
        if (rc != DS2I_OK) return rc;
        sh->idx.reset(raw);
        sh->term_map.assign(src[s].term_map, src[s].term_map + nlists[s]);
        std::vector<uint32_t> df(nlists[s]);
        for (uint64_t j = 0; j < nlists[s]; ++j) df[j] = (uint32_t)(stats_df ? stats_df[sh->term_map[j]] : df_sum[sh->term_map[j]]);
        rc = ds2i_hip_index_set_collection_stats(raw, num_docs, df.data(), df.size());
        if (rc != DS2I_OK) return rc;
        ds2i_hip_pipeline* p = nullptr;
        rc = ds2i_hip_pipeline_create(raw, 1, &p);
        if (rc != DS2I_OK) return rc;
        sh->pipe.reset(p);
        set->shards.push_back(std::move(sh));
    }
    if (!set->shards.empty()) {
        int rc = set->merge.open("ds2i_hip_shard_set_open", set->shards[0]->device, (uint32_t)set->shards.size());
        for (size_t i = 0; i < set->shards.size() && rc == DS2I_OK; ++i) {
            const ds2i_shard_source& so = src[set->shards[i]->source];
            rc = set->merge.set_map("ds2i_hip_shard_set_open", (uint32_t)i, so.doc_map, so.map_len);
        }
        if (rc != DS2I_OK) return rc;
    }
    *out = set.release();
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_shard_set_query(ds2i_hip_shard_set* s, int op, uint32_t k, const uint32_t* terms, const uint32_t* query_offsets, uint32_t nq,
                             uint64_t* out_count, float* out_topk, uint32_t* out_topk_docs, uint32_t* out_topk_len, ds2i_hip_shard_stats* stats) {
    static const std::string who = "ds2i_hip_shard_set_query: ";
    if (!s || !query_offsets || (!terms && nq && query_offsets[nq])) return ds2i_set_error(DS2I_EINVAL, (who + "null argument").c_str());
    const int base = op & 0xFF;
    if (op & ~(0xFF | DS2I_OP_TOPK_DOCS))
        return ds2i_set_error(DS2I_EINVAL, (who + "DS2I_OP_TOPK_DOCS is the one flag a shard set takes (DS2I_OP_REFERENCE_ORDER is not offered)").c_str());
    const bool ranked = base >= DS2I_OP_RANKED_AND && base <= DS2I_OP_RANKED_OR;
    if (!ranked && base != DS2I_OP_AND && base != DS2I_OP_OR)
        return ds2i_set_error(DS2I_EINVAL, (who + "a shard set answers and, or and the four ranked operators (and_freq / or_freq are not merged)").c_str());
    if (!ranked && (op & DS2I_OP_TOPK_DOCS)) return ds2i_set_error(DS2I_EINVAL, (who + "and / or have no top-k").c_str());
    if (ranked && (k == 0 || k > DS2I_HIP_MAX_K_LONG))
        return ds2i_set_error(DS2I_EINVAL, (who + "k = " + std::to_string(k) + " lies outside 1 .. " + std::to_string(DS2I_HIP_MAX_K_LONG)).c_str());
    if (nq && (ranked ? (!out_topk || !out_topk_docs) : !out_count)) return ds2i_set_error(DS2I_EINVAL, (who + "null output").c_str());
    for (uint32_t q = 0; q < nq; ++q)
        if (query_offsets[q + 1] < query_offsets[q]) return ds2i_set_error(DS2I_EINVAL, (who + "query_offsets must be non-decreasing").c_str());
    for (uint32_t i = nq ? query_offsets[0] : 0; nq && i < query_offsets[nq]; ++i)
        if (terms[i] >= s->collection_terms) return ds2i_set_error(DS2I_ETERM, "term id out of range");
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (stats) stats->shards_open = (uint32_t)s->shards.size();
    if (!nq) return DS2I_OK;
    DS2I_TRY
    const size_t n = s->shards.size();
    const bool conj = base == DS2I_OP_AND || base == DS2I_OP_RANKED_AND;
    const auto t0 = std::chrono::steady_clock::now();
    ds2i_host::parallel_for(n, (unsigned)std::min<size_t>(n, 16), [&](uint64_t i, unsigned) {
        Shard& sh = *s->shards[i];
        sh.terms.clear();
        sh.offs.assign(nq + 1, 0);
        for (uint32_t q = 0; q < nq; ++q) {
            ds2i_host::translate_query(terms + query_offsets[q], query_offsets[q + 1] - query_offsets[q], sh.term_map.data(), sh.term_map.size(), conj,
                                       sh.terms);
            sh.offs[q + 1] = (uint32_t)sh.terms.size();
        }
        if (sh.terms.empty()) sh.terms.push_back(0); // (never read: every query is empty)
        sh.count.assign(nq, 0);
        if (ranked) {
            sh.topk.resize((size_t)nq * k);
            sh.docs.resize((size_t)nq * k);
            sh.lens.assign(nq, 0);
        }
    }, true);
    if (stats) stats->translate_ms = ms_since(t0);
    const int shard_op = base | (ranked ? (int)DS2I_OP_TOPK_DOCS : 0);
    int rc = DS2I_OK;
    std::string err;
    for (size_t i = 0; i < n && rc == DS2I_OK; ++i) {
        Shard& sh = *s->shards[i];
        rc = ds2i_hip_pipeline_submit(sh.pipe.get(), shard_op, k, sh.terms.data(), sh.offs.data(), nq, &sh.ticket);
        sh.in_flight = rc == DS2I_OK;
        if (rc != DS2I_OK) err = ds2i_get_error();
    }
    for (size_t i = 0; i < n; ++i) { // every submitted ticket is collected, whatever happened to the others
        Shard& sh = *s->shards[i];
        if (!sh.in_flight) continue;
        sh.in_flight = false;
        ds2i_hip_stats st{};
        const int wrc = ranked ? ds2i_hip_pipeline_wait_docs(sh.pipe.get(), sh.ticket, sh.count.data(), sh.topk.data(), sh.docs.data(), sh.lens.data(), &st)
                               : ds2i_hip_pipeline_wait(sh.pipe.get(), sh.ticket, sh.count.data(), nullptr, nullptr, &st);
        if (wrc != DS2I_OK && rc == DS2I_OK) {
            rc = wrc;
            err = ds2i_get_error();
        }
        if (stats) stats->kernel_ms[sh.source] = st.kernel_ms;
    }
    if (rc != DS2I_OK) return ds2i_set_error(rc, err.c_str());
    if (!ranked) {
        for (uint32_t q = 0; q < nq; ++q) {
            uint64_t sum = 0;
            for (size_t i = 0; i < n; ++i) sum += s->shards[i]->count[q];
            out_count[q] = sum;
        }
        return DS2I_OK;
    }
    std::vector<uint32_t> lens(nq, 0);
    if (n == 0) { // every shard was skipped: every row is empty
        for (size_t i = 0; i < (size_t)nq * k; ++i) {
            out_topk[i] = -std::numeric_limits<float>::infinity();
            out_topk_docs[i] = 0xFFFFFFFFu;
        }
    } else {
        std::vector<ds2i_topk_rows> rows(n);
        for (size_t i = 0; i < n; ++i) {
            const Shard& sh = *s->shards[i];
            rows[i] = ds2i_topk_rows{sh.topk.data(), sh.docs.data(), sh.lens.data(), nullptr, 0}; // (the maps are on the merge device)
        }
        double ms = 0.0;
        rc = s->merge.run("ds2i_hip_shard_set_query", rows.data(), (uint32_t)n, nq, k, out_topk, out_topk_docs, lens.data(), ms);
        if (rc != DS2I_OK) return rc;
        if (stats) stats->merge_ms = ms;
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (out_topk_len) out_topk_len[q] = lens[q];
        if (out_count) out_count[q] = lens[q];
    }
    return DS2I_OK;
    DS2I_CATCH
}

void ds2i_hip_shard_set_close(ds2i_hip_shard_set* s) {
    if (!s) return;
    for (auto& sh : s->shards) { // the pipeline goes before its index
        (void)hipSetDevice(sh->device);
        sh->pipe.reset();
        sh->idx.reset();
    }
    delete s;
}

} // extern "C"
