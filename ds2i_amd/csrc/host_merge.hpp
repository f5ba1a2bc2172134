// host_merge.hpp -- the host's side of merging collections (no HIP): every check of a merge's arguments, the plan that says where each
// source list's run of postings starts inside its merged list, and the host twin of the device merge (every run placed, every merged
// list sorted by doc-id with its freqs). The device entry points (capi_merge.cpp) make the same plan from the same checks.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_parallel.hpp"
#include "host_remap.hpp"

namespace ds2i_host {

// one source as the plan sees it: its shape and its maps, no postings
struct merge_shape {
    uint64_t num_docs = 0, nlists = 0;
    const uint64_t* offs = nullptr;     // nlists + 1 posting offsets, from 0
    const uint32_t* doc_map = nullptr;  // null: base + old doc-id, base = the documents of the earlier sources
    uint64_t map_len = 0;               // (looked at only beside a map)
    const uint32_t* term_map = nullptr; // null: the identity
    uint64_t terms_len = 0;
};

struct merge_plan {
    uint64_t num_docs = 0, nlists = 0;
    bool identity = true;                         // the concatenated doc maps are the identity: every merged list is sorted as placed
    std::vector<uint64_t> base;                   // per source: the documents before it
    std::vector<uint64_t> offs;                   // nlists + 1: the merged lists
    std::vector<std::vector<uint64_t>> dst_first; // per source and source list: where its run starts among the merged postings
    uint64_t merged_term(const merge_shape& s, uint64_t t) const { return s.term_map ? s.term_map[t] : t; }
};

// "" and the shapes of sources given in CSR form (Src: ds2i_merge_postings_source of ds2i_build.h), or the null pointer or the offsets
// that are wrong
template <class Src>
std::string merge_csr_fault(const char* who_, const Src* src, uint32_t nsrc, std::vector<merge_shape>& shapes) {
    const std::string who = std::string(who_) + ": ";
    if (!src) return who + "null argument";
    shapes.assign(nsrc, merge_shape());
    for (uint32_t s = 0; s < nsrc; ++s) {
        if (!src[s].list_offsets || !src[s].docs || !src[s].freqs) return who + "null argument";
        if (src[s].list_offsets[0] != 0) return who + "list_offsets must start at 0";
        for (uint64_t t = 0; t < src[s].nlists; ++t)
            if (src[s].list_offsets[t + 1] < src[s].list_offsets[t]) return who + "list_offsets decrease";
        merge_shape& m = shapes[s];
        m.num_docs = src[s].num_docs;
        m.nlists = src[s].nlists;
        m.offs = src[s].list_offsets;
        m.doc_map = src[s].doc_map;
        m.map_len = src[s].map_len;
        m.term_map = src[s].term_map;
        m.terms_len = src[s].terms_len;
    }
    return "";
}

// "" and the plan, or what is wrong with the arguments, in this order: no source; 2^32 documents or lists; a map of the wrong length;
// the doc maps, defaults filled in and concatenated in source order, no permutation of all documents (doc_map_fault's text, the
// document numbered in the concatenation); a term map that does not increase strictly or leaves [0, nlists); a merged term that no
// source list maps to. nlists == 0 asks for the smallest number of lists that holds every mapped term. Runs are placed in source order.
inline std::string merge_plan_fault(const char* who_, const merge_shape* src, uint32_t nsrc, uint64_t nlists, merge_plan& p) {
    const std::string who = std::string(who_) + ": ";
    if (!nsrc) return who + "no source";
    p.base.assign(nsrc, 0);
    uint64_t docs = 0, want_lists = 0;
    bool any_map = false;
    for (uint32_t s = 0; s < nsrc; ++s) {
        const merge_shape& m = src[s];
        p.base[s] = docs;
        docs += m.num_docs;
        if (docs >= (1ull << 32) || m.nlists >= (1ull << 32) || nlists >= (1ull << 32)) return who + "2^32 documents or lists, or more";
        if (m.doc_map && m.map_len != m.num_docs)
            return who + "the doc map of source " + std::to_string(s) + " holds " + std::to_string(m.map_len) + " documents, the source " +
                   std::to_string(m.num_docs);
        if (m.term_map && m.terms_len != m.nlists)
            return who + "the term map of source " + std::to_string(s) + " holds " + std::to_string(m.terms_len) + " terms, the source " +
                   std::to_string(m.nlists) + " lists";
        any_map = any_map || m.doc_map;
    }
    p.num_docs = docs;
    p.identity = true;
    if (any_map) {
        std::vector<uint32_t> all(docs);
        for (uint32_t s = 0; s < nsrc; ++s)
            for (uint64_t d = 0; d < src[s].num_docs; ++d) {
                const uint64_t v = src[s].doc_map ? src[s].doc_map[d] : p.base[s] + d;
                all[p.base[s] + d] = (uint32_t)v;
                p.identity = p.identity && v == p.base[s] + d;
            }
        const std::string fault = doc_map_fault(all.data(), docs);
        if (!fault.empty()) return who + "the doc maps, concatenated, are no permutation: " + fault;
    }
    for (uint32_t s = 0; s < nsrc; ++s) {
        const merge_shape& m = src[s];
        if (!m.nlists) continue;
        if (m.term_map)
            for (uint64_t t = 1; t < m.nlists; ++t)
                if (m.term_map[t] <= m.term_map[t - 1])
                    return who + "the term map of source " + std::to_string(s) + " does not increase at list " + std::to_string(t);
        const uint64_t last = p.merged_term(m, m.nlists - 1);
        if (nlists && last >= nlists)
            return who + "the term map of source " + std::to_string(s) + " sends list " + std::to_string(m.nlists - 1) + " to term " +
                   std::to_string(last) + ", outside the " + std::to_string(nlists) + " merged lists";
        want_lists = std::max(want_lists, last + 1);
    }
    p.nlists = nlists ? nlists : want_lists;
    p.offs.assign(p.nlists + 1, 0);
    std::vector<uint8_t> seen(p.nlists, 0);
    for (uint32_t s = 0; s < nsrc; ++s)
        for (uint64_t t = 0; t < src[s].nlists; ++t) {
            const uint64_t to = p.merged_term(src[s], t);
            p.offs[to + 1] += src[s].offs[t + 1] - src[s].offs[t];
            seen[to] = 1;
        }
    for (uint64_t t = 0; t < p.nlists; ++t) {
        if (!seen[t]) return who + "merged term " + std::to_string(t) + " receives no list: List must be nonempty";
        p.offs[t + 1] += p.offs[t];
    }
    std::vector<uint64_t> next(p.offs.begin(), p.offs.end() - 1); // where the next run of every merged list goes
    p.dst_first.assign(nsrc, {});
    for (uint32_t s = 0; s < nsrc; ++s) {
        p.dst_first[s].resize(src[s].nlists);
        for (uint64_t t = 0; t < src[s].nlists; ++t) {
            const uint64_t to = p.merged_term(src[s], t);
            p.dst_first[s][t] = next[to];
            next[to] += src[s].offs[t + 1] - src[s].offs[t];
        }
    }
    return "";
}

// The twin: out_docs / out_freqs hold p.offs[p.nlists] words each. Every source's runs are placed where the plan says, the doc-ids through
// the source's map (or its base added); then, unless the maps are the identity, every merged list is sorted by doc-id, the freqs with
// it. A doc-id at or past a source's number of documents throws (nothing is read past a map).
inline void merge_postings(const merge_shape* src, const uint32_t* const* docs, const uint32_t* const* freqs, uint32_t nsrc, merge_plan const& p,
                           uint32_t* out_docs, uint32_t* out_freqs, unsigned threads) {
    for (uint32_t s = 0; s < nsrc; ++s) {
        const merge_shape& m = src[s];
        parallel_for(m.nlists, threads, [&](uint64_t t, unsigned) {
            const uint64_t first = m.offs[t], n = m.offs[t + 1] - first, to = p.dst_first[s][t];
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t d = docs[s][first + i];
                if (d >= m.num_docs)
                    throw std::runtime_error("ds2i_merge_postings: list " + std::to_string(t) + " of source " + std::to_string(s) + " holds doc-id " +
                                             std::to_string(d) + ", outside the map");
                out_docs[to + i] = m.doc_map ? m.doc_map[d] : (uint32_t)(p.base[s] + d);
                out_freqs[to + i] = freqs[s][first + i];
            }
        });
    }
    if (p.identity) return;
    std::vector<std::vector<uint64_t>> scratch(threads ? threads : 1);
    parallel_for(p.nlists, threads, [&](uint64_t t, unsigned w) {
        const uint64_t first = p.offs[t], n = p.offs[t + 1] - first;
        std::vector<uint64_t>& pairs = scratch[w];
        pairs.resize(n);
        for (uint64_t i = 0; i < n; ++i) pairs[i] = (uint64_t)out_docs[first + i] << 32 | out_freqs[first + i];
        std::sort(pairs.begin(), pairs.end());
        for (uint64_t i = 0; i < n; ++i) {
            out_docs[first + i] = (uint32_t)(pairs[i] >> 32);
            out_freqs[first + i] = (uint32_t)pairs[i];
        }
    });
}

} // namespace ds2i_host
