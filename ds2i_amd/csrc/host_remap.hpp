// host_remap.hpp -- the host's side of renumbering documents (no HIP): the check that a doc-id map is a permutation, the host twin of the
// device remap (every doc-id through the map, every list sorted again with its freqs), and the wand image of a renumbered collection.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_index.hpp"
#include "host_parallel.hpp"

namespace ds2i_host {

// "" when doc_map is a permutation of [0, num_docs); else what the FIRST offending old doc-id does: it maps to a value >= num_docs, or to
// an id an earlier document took. One bit per document.
inline std::string doc_map_fault(const uint32_t* doc_map, uint64_t num_docs) {
    std::vector<uint64_t> taken((num_docs + 63) / 64, 0);
    for (uint64_t d = 0; d < num_docs; ++d) {
        const uint64_t v = doc_map[d];
        if (v >= num_docs)
            return "document " + std::to_string(d) + " maps to " + std::to_string(v) + ", outside the " + std::to_string(num_docs) + " documents";
        if (taken[v >> 6] >> (v & 63) & 1) return "document " + std::to_string(d) + " maps to " + std::to_string(v) + ", which an earlier document took";
        taken[v >> 6] |= 1ull << (v & 63);
    }
    return "";
}

// list t = docs / freqs [offs[t], offs[t + 1]) in place: docs through the map, then the pairs sorted by new doc-id. A doc-id outside the
// map throws (nothing is read past the map; lists already done stay remapped).
inline void remap_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* offs, uint32_t* docs, uint32_t* freqs, const uint32_t* doc_map,
                           unsigned threads) {
    std::vector<std::vector<uint64_t>> scratch(threads ? threads : 1);
    parallel_for(nlists, threads, [&](uint64_t t, unsigned w) {
        const uint64_t first = offs[t], n = offs[t + 1] - first;
        std::vector<uint64_t>& pairs = scratch[w];
        pairs.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            if (docs[first + i] >= num_docs)
                throw std::runtime_error("ds2i_remap_postings: list " + std::to_string(t) + " holds doc-id " + std::to_string(docs[first + i]) +
                                         ", outside the map");
            pairs[i] = (uint64_t)doc_map[docs[first + i]] << 32 | freqs[first + i];
        }
        std::sort(pairs.begin(), pairs.end());
        for (uint64_t i = 0; i < n; ++i) {
            docs[first + i] = (uint32_t)(pairs[i] >> 32);
            freqs[first + i] = (uint32_t)pairs[i];
        }
    });
}

// The wand image of the renumbered collection without a pass over the postings: norm_lens permuted, max_term_weight copied. The bytes are
// those of a build from scratch: compute_norm_lens sums integer-valued floats in a double, so the average does not depend on the order
// of the documents, and a term's maximum is taken over the same set of floats. (The caller has checked the map against w.num_docs.)
inline void remap_wand(wand_view const& w, const uint32_t* doc_map, bytes_t& out) {
    std::vector<float> norm_lens(w.num_docs), max_w(w.num_terms);
    for (uint64_t d = 0; d < w.num_docs; ++d) std::memcpy(&norm_lens[doc_map[d]], w.norm_lens + 4 * d, 4);
    if (w.num_terms) std::memcpy(max_w.data(), w.max_term_weight, 4 * w.num_terms);
    wand_freeze(norm_lens, max_w, out);
}

} // namespace ds2i_host
