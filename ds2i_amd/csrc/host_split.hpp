// host_split.hpp -- the host's side of splitting a collection by documents (no HIP), the inverse of host_merge.hpp: every check of a
// split's arguments, the tables every shard shares (the local id of every document, every shard's doc map) and the host twin of the
// device split. The device entry points (capi_split.cpp) make the same checks and the same tables.
//
// shard_of[d] < nshards names the shard of document d, SPLIT_DROP deletes it. The documents of a shard keep their order: the local id of
// a document is its rank among them, doc_map[local id] its old id. A list survives in a shard when one of its postings lies in a document
// of the shard; surviving lists keep their order (term_map[list of the shard] = old term), their postings keep theirs, and nothing is
// ever sorted. The maps are the ones merge_plan_fault (host_merge.hpp) takes.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_parallel.hpp"

namespace ds2i_host {

constexpr uint32_t SPLIT_DROP = 0xFFFFFFFFu;

struct split_shard {
    uint64_t num_docs = 0, nlists = 0;
    std::vector<uint32_t> doc_map, term_map; // num_docs old doc-ids, nlists old terms, both strictly increasing
    std::vector<uint64_t> offs;              // nlists + 1 posting offsets, from 0
    std::vector<uint32_t> docs, freqs;       // offs[nlists] postings, the doc-ids local
};

// "" or what is wrong with offsets that are not null (the CSR entry points; an image's offsets come from its parse)
inline std::string split_csr_fault(const char* who_, uint64_t nlists, const uint64_t* offs) {
    const std::string who = std::string(who_) + ": ";
    if (offs[0] != 0) return who + "list_offsets must start at 0";
    for (uint64_t t = 0; t < nlists; ++t)
        if (offs[t + 1] < offs[t]) return who + "list_offsets decrease";
    return "";
}

// "" or what is wrong, in this order: no shard; 2^32 documents or lists; the FIRST document whose value is neither a shard nor the drop
// value. No posting is looked at.
inline std::string split_assign_fault(const char* who_, uint64_t num_docs, uint64_t nlists, const uint32_t* shard_of, uint32_t nshards) {
    const std::string who = std::string(who_) + ": ";
    if (!nshards) return who + "no shard";
    if (num_docs >= (1ull << 32) || nlists >= (1ull << 32)) return who + "2^32 documents or lists, or more";
    for (uint64_t d = 0; d < num_docs; ++d)
        if (shard_of[d] >= nshards && shard_of[d] != SPLIT_DROP)
            return who + "document " + std::to_string(d) + " is sent to shard " + std::to_string(shard_of[d]) + ", outside the " +
                   std::to_string(nshards) + " shards";
    return "";
}

// One pass over a checked shard_of: local[d] = the rank of d among the documents of its shard (0 for a dropped one, which nothing reads),
// doc_maps[s] = the old ids of shard s in increasing order.
inline void split_tables(uint64_t num_docs, const uint32_t* shard_of, uint32_t nshards, std::vector<uint32_t>& local,
                         std::vector<std::vector<uint32_t>>& doc_maps) {
    std::vector<uint64_t> count(nshards, 0);
    for (uint64_t d = 0; d < num_docs; ++d)
        if (shard_of[d] != SPLIT_DROP) ++count[shard_of[d]];
    doc_maps.assign(nshards, {});
    for (uint32_t s = 0; s < nshards; ++s) doc_maps[s].reserve(count[s]);
    local.assign(num_docs, 0);
    for (uint64_t d = 0; d < num_docs; ++d)
        if (shard_of[d] != SPLIT_DROP) {
            local[d] = (uint32_t)doc_maps[shard_of[d]].size();
            doc_maps[shard_of[d]].push_back((uint32_t)d);
        }
}

// What the host makes of a shard's kept-postings counts, on either side: kept_before[t] = the shard's postings before source list t
// (nlists + 1 values, the last the shard's total). Lists whose two consecutive values are equal vanish: the rest give the term map and
// the shard's offsets.
inline void split_shard_lists(uint64_t nlists, const uint64_t* kept_before, split_shard& out) {
    out.term_map.clear();
    out.offs.assign(1, 0);
    for (uint64_t t = 0; t < nlists; ++t)
        if (kept_before[t + 1] != kept_before[t]) {
            out.term_map.push_back((uint32_t)t);
            out.offs.push_back(kept_before[t + 1]);
        }
    out.nlists = out.term_map.size();
}

// The twin: out[s] is shard s. Arguments as the two fault functions left them. List-parallel, a shard at a time: the kept postings of
// every list are counted, the counts scanned, and every list's kept postings stored behind those of the lists before it. A doc-id at or
// past num_docs throws while the first shard is counted (nothing is read past shard_of, and `out` is written only once no list threw).
inline void split_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs, const uint32_t* freqs,
                           const uint32_t* shard_of, uint32_t nshards, unsigned threads, std::vector<split_shard>& out) {
    std::vector<uint32_t> local;
    std::vector<std::vector<uint32_t>> doc_maps;
    split_tables(num_docs, shard_of, nshards, local, doc_maps);
    std::vector<split_shard> shards(nshards);
    std::vector<uint64_t> kept_before(nlists + 1);
    for (uint32_t s = 0; s < nshards; ++s) {
        split_shard& sh = shards[s];
        kept_before[0] = 0;
        parallel_for(nlists, threads, [&](uint64_t t, unsigned) {
            uint64_t kept = 0;
            for (uint64_t i = offs[t]; i < offs[t + 1]; ++i) {
                const uint64_t d = docs[i];
                if (d >= num_docs)
                    throw std::runtime_error("ds2i_split_postings: list " + std::to_string(t) + " holds doc-id " + std::to_string(d) +
                                             ", outside the " + std::to_string(num_docs) + " documents");
                kept += shard_of[d] == s;
            }
            kept_before[t + 1] = kept;
        });
        for (uint64_t t = 0; t < nlists; ++t) kept_before[t + 1] += kept_before[t];
        split_shard_lists(nlists, kept_before.data(), sh);
        sh.docs.resize(kept_before[nlists]);
        sh.freqs.resize(kept_before[nlists]);
        parallel_for(nlists, threads, [&](uint64_t t, unsigned) {
            uint64_t to = kept_before[t];
            for (uint64_t i = offs[t]; i < offs[t + 1]; ++i) {
                const uint32_t d = docs[i];
                if (shard_of[d] != s) continue;
                sh.docs[to] = local[d];
                sh.freqs[to++] = freqs[i];
            }
        });
        sh.num_docs = doc_maps[s].size();
        sh.doc_map.swap(doc_maps[s]);
    }
    out.swap(shards);
}

} // namespace ds2i_host
