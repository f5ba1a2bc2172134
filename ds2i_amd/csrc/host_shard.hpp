// host_shard.hpp -- the host's side of querying document shards as one index (no HIP): the wand data of a shard under the collection's
// normalisation, the key order of a merge of top-k rows with every check of its arguments, the host twin of the device merge
// (shard_kernels.hip), and the translation of a query's collection terms into a shard's local terms. include/ds2i_build.h states the
// semantics; capi_build.cpp and capi_shards.cpp are the entry points.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/ds2i_build.h"
#include "host_index.hpp"
#include "host_parallel.hpp"

namespace ds2i_host {

constexpr uint32_t SHARD_MAX_ROWS = 64;    // DS2I_HIP_MAX_SHARDS
constexpr uint32_t SHARD_MAX_K = 1024;     // DS2I_HIP_MAX_K_LONG
constexpr uint32_t TOPK_NO_DOC = 0xFFFFFFFFu;

// ------------------------------------------------------------ wand data
// "" or the first map entry past the image's arrays
inline std::string split_wand_fault(const char* who, wand_view const& w, const uint32_t* doc_map, uint64_t ndocs, const uint32_t* term_map,
                                    uint64_t nterms) {
    for (uint64_t i = 0; i < ndocs; ++i)
        if (doc_map[i] >= w.num_docs)
            return std::string(who) + ": doc_map[" + std::to_string(i) + "] = " + std::to_string(doc_map[i]) + " lies outside the " +
                   std::to_string(w.num_docs) + " documents of the wand data";
    for (uint64_t j = 0; j < nterms; ++j)
        if (term_map[j] >= w.num_terms)
            return std::string(who) + ": term_map[" + std::to_string(j) + "] = " + std::to_string(term_map[j]) + " lies outside the " +
                   std::to_string(w.num_terms) + " terms of the wand data";
    return "";
}

// both arrays gathered through the (checked) maps: the collection's normalisation, NOT what a build over the shard gives
inline void split_wand(wand_view const& w, const uint32_t* doc_map, uint64_t ndocs, const uint32_t* term_map, uint64_t nterms, bytes_t& out) {
    std::vector<float> norm_lens(ndocs), max_w(nterms);
    for (uint64_t i = 0; i < ndocs; ++i) std::memcpy(&norm_lens[i], w.norm_lens + 4 * (uint64_t)doc_map[i], 4);
    for (uint64_t j = 0; j < nterms; ++j) std::memcpy(&max_w[j], w.max_term_weight + 4 * (uint64_t)term_map[j], 4);
    wand_freeze(norm_lens, max_w, out);
}

// ------------------------------------------------------------ merging top-k rows
inline uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
// the key of a candidate: ascending key = score descending, equal scores by collection doc-id ascending
inline uint64_t topk_key(uint32_t score_bits, uint32_t g) { return (uint64_t)(0xFFFFFFFFu - score_bits) << 32 | g; }
inline float topk_key_score(uint64_t key) {
    const uint32_t u = 0xFFFFFFFFu - (uint32_t)(key >> 32);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

inline bool map_increases(const uint32_t* m, uint64_t n) {
    for (uint64_t i = 1; i < n; ++i)
        if (m[i] <= m[i - 1]) return false;
    return true;
}

// "" or what is wrong, in the header's order: null arguments; the number of row sets; k; the first lens[q] > k; the first candidate
// whose score is negative or not finite; the first candidate whose local id lies outside its map. `outputs_null`: the caller's outputs.
inline std::string merge_topk_fault(const char* who_, const ds2i_topk_rows* rows, uint32_t nrows, uint32_t nq, uint32_t k, bool outputs_null) {
    const std::string who = std::string(who_) + ": ";
    if (!rows || outputs_null) return who + "null argument";
    if (nq)
        for (uint32_t r = 0; r < nrows && r < SHARD_MAX_ROWS; ++r)
            if (!rows[r].scores || !rows[r].docs || !rows[r].lens || (!rows[r].doc_map && rows[r].map_len)) return who + "null argument";
    if (nrows == 0 || nrows > SHARD_MAX_ROWS) return who + std::to_string(nrows) + " row sets: 1 to " + std::to_string(SHARD_MAX_ROWS) + " are merged";
    if (k == 0 || k > SHARD_MAX_K) return who + "k = " + std::to_string(k) + " lies outside 1 .. " + std::to_string(SHARD_MAX_K);
    auto at = [&](uint32_t r, uint32_t q) { return "row set " + std::to_string(r) + ", query " + std::to_string(q); };
    for (uint32_t r = 0; r < nrows; ++r)
        for (uint32_t q = 0; q < nq; ++q)
            if (rows[r].lens[q] > k) return who + at(r, q) + ": length " + std::to_string(rows[r].lens[q]) + " is above k = " + std::to_string(k);
    for (uint32_t r = 0; r < nrows; ++r)
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = 0; i < rows[r].lens[q]; ++i) {
                const uint32_t u = float_bits(rows[r].scores[(uint64_t)q * k + i]);
                if (u >= 0x7F800000u) // the sign bit, an infinity or a NaN
                    return who + at(r, q) + ", position " + std::to_string(i) + ": the score is negative or not finite";
            }
    for (uint32_t r = 0; r < nrows; ++r) {
        if (!rows[r].doc_map) continue;
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = 0; i < rows[r].lens[q]; ++i) {
                const uint32_t doc = rows[r].docs[(uint64_t)q * k + i];
                if (doc >= rows[r].map_len)
                    return who + at(r, q) + ", position " + std::to_string(i) + ": local doc-id " + std::to_string(doc) + " lies outside the map of " +
                           std::to_string(rows[r].map_len);
            }
    }
    return "";
}

// the twin: per query every candidate's key, sorted, the first k written out and the row padded. Arguments checked by the caller.
inline void merge_topk(const ds2i_topk_rows* rows, uint32_t nrows, uint32_t nq, uint32_t k, float* out_scores, uint32_t* out_docs,
                       uint32_t* out_lens, unsigned threads) {
    std::vector<std::vector<uint64_t>> scratch(threads ? threads : 1);
    const float ninf = -std::numeric_limits<float>::infinity();
    parallel_for(nq, threads, [&](uint64_t q, unsigned w) {
        std::vector<uint64_t>& keys = scratch[w];
        keys.clear();
        for (uint32_t r = 0; r < nrows; ++r)
            for (uint32_t i = 0; i < rows[r].lens[q]; ++i) {
                const uint32_t doc = rows[r].docs[q * k + i];
                keys.push_back(topk_key(float_bits(rows[r].scores[q * k + i]), rows[r].doc_map ? rows[r].doc_map[doc] : doc));
            }
        std::sort(keys.begin(), keys.end());
        const uint32_t n = (uint32_t)std::min<uint64_t>(k, keys.size());
        for (uint32_t i = 0; i < k; ++i) {
            out_scores[q * k + i] = i < n ? topk_key_score(keys[i]) : ninf;
            out_docs[q * k + i] = i < n ? (uint32_t)keys[i] : TOPK_NO_DOC;
        }
        out_lens[q] = n;
    }, true);
}

// ------------------------------------------------------------ a query's terms in a shard
// The terms of one query (collection term ids, repeats kept: they are the query term frequencies) as the local terms of a shard whose
// term_map (strictly increasing) holds `nterms` collection terms, appended to `out`. conjunctive: a distinct term the shard does not hold
// makes the query the empty query (nothing is appended); else absent terms are dropped.
inline void translate_query(const uint32_t* terms, uint32_t n, const uint32_t* term_map, uint64_t nterms, bool conjunctive, std::vector<uint32_t>& out) {
    const size_t begin = out.size();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t* p = std::lower_bound(term_map, term_map + nterms, terms[i]);
        if (p != term_map + nterms && *p == terms[i])
            out.push_back((uint32_t)(p - term_map));
        else if (conjunctive) {
            out.resize(begin);
            return;
        }
    }
}

} // namespace ds2i_host
