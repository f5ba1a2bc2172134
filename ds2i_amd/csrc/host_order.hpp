// host_order.hpp -- the host's side of ordering documents by recursive graph bisection (no HIP): the argument checks, the fixed-point
// logarithm table, the integer cost of a collection's gaps, and the host twin of the device ordering (capi_order.cpp,
// order_kernels.hip), which returns the same map and the same trace element for element. The shared arithmetic is order_cost.hpp's.
//
// The algorithm. The input is the postings of a collection: nlists strictly increasing doc-id lists over num_docs documents. The output
// is doc_map, a permutation of [0, num_docs) with new id = doc_map[old id] (what a remap takes), and a trace of one u64 per (level,
// iteration) that ran: the exchanges of that iteration.
//   order[s] is the document at position s; it starts as the identity. Level l runs iff l < max_levels and every level l + 1 segment
//   holds at least min_half documents; the first level that fails ends the run. At a level's start every document is named by its
//   position then, p0, and members[s] = s; during the level only members changes, and the side of a p0 is the half its slot lies in.
//   One iteration, of at most `iterations`: (1) for every term and level l segment, dl and dr: the term's documents now in the left and
//   the right half; (2) for every document the sum of order_term_cost over its terms as int64, clamped to int32: its gain; (3) each
//   half's members sorted by gain descending, equal gains by smaller p0 first; (4) in each segment, with m = min(|left|, |right|), the
//   i-th left and the i-th right member exchanged for every i < m with gain_left[i] + gain_right[i] > 0; (5) the exchanges counted:
//   zero ends the level. At a level's end order'[s] = order[members[s]]; at the end of the run doc_map[order[s]] = s.
// The twin keeps the lists in p0 order (every list through the level's map, sorted again: remap_postings), so a term's documents of one
// segment are one run of its list, as on the device; it needs no forward index.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "host_parallel.hpp"
#include "host_remap.hpp"
#include "order_cost.hpp"

namespace ds2i_host {

struct order_params {
    uint32_t iterations = ORDER_DEFAULT_ITERATIONS, min_half = ORDER_DEFAULT_MIN_HALF, max_levels = ORDER_DEFAULT_MAX_LEVELS;
};

// LOGQ[x]: the one place a logarithm is taken
inline uint32_t order_logq(uint64_t x) { return x ? (uint32_t)std::rint(std::log2((double)x) * (double)(1u << ORDER_FRAC_BITS)) : 0u; }
// out[x] = LOGQ[x] for x < n
inline void order_log_table(uint64_t n, uint32_t* out) {
    for (uint64_t x = 0; x < n; ++x) out[x] = order_logq(x);
}

// "" or what is wrong with the offsets of a CSR input whose pointers are not null
inline std::string order_offsets_fault(const char* who_, uint64_t nlists, const uint64_t* offs) {
    const std::string who = std::string(who_) + ": ";
    if (offs[0] != 0) return who + "list_offsets must start at 0";
    for (uint64_t t = 0; t < nlists; ++t)
        if (offs[t + 1] < offs[t]) return who + "list_offsets decrease";
    return "";
}
// "" or the first list that holds a doc-id >= num_docs or does not strictly increase
inline std::string order_docs_fault(const char* who_, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs) {
    for (uint64_t t = 0; t < nlists; ++t)
        for (uint64_t i = offs[t]; i < offs[t + 1]; ++i) {
            if (docs[i] >= num_docs)
                return std::string(who_) + ": list " + std::to_string(t) + " holds doc-id " + std::to_string(docs[i]) + ", outside the " +
                       std::to_string(num_docs) + " documents";
            if (i > offs[t] && docs[i - 1] >= docs[i])
                return std::string(who_) + ": the doc-ids of list " + std::to_string(t) + " do not strictly increase at position " + std::to_string(i - offs[t]);
        }
    return "";
}
inline std::string order_num_docs_fault(const char* who_, uint64_t num_docs) {
    return num_docs >= ORDER_MAX_DOCS ? std::string(who_) + ": 2^32 - 2 documents or more" : "";
}
// "" or the parameter out of bounds; zeros become the defaults in `out`
inline std::string order_params_fault(const char* who_, uint32_t iterations, uint32_t min_half, uint32_t max_levels, order_params& out) {
    out = order_params();
    if (iterations > ORDER_MAX_ITERATIONS) return std::string(who_) + ": iterations above " + std::to_string(ORDER_MAX_ITERATIONS);
    if (max_levels > ORDER_MAX_LEVELS) return std::string(who_) + ": max_levels above " + std::to_string(ORDER_MAX_LEVELS);
    if (iterations) out.iterations = iterations;
    if (min_half) out.min_half = min_half;
    if (max_levels) out.max_levels = max_levels;
    return "";
}

// level l runs: l < max_levels and every level l + 1 segment holds min_half documents or more. The smallest segment of a level holds
// floor(n / 2^level) documents (segment 0 does).
inline bool order_level_runs(uint64_t n, uint32_t level, order_params const& p) {
    if (level >= p.max_levels) return false; // (max_levels <= 32: the shift below is by 32 at most)
    return (n >> (level + 1)) >= p.min_half;
}

// sum of LOGQ[gap] over all postings of checked lists (strictly increasing), a list's first gap being doc + 1: an exact integer
inline uint64_t postings_cost(uint64_t nlists, const uint64_t* offs, const uint32_t* docs) {
    std::vector<uint32_t> small(1u << 16); // the gaps that occur most, looked up; the rest evaluated
    order_log_table(small.size(), small.data());
    uint64_t cost = 0;
    for (uint64_t t = 0; t < nlists; ++t)
        for (uint64_t i = offs[t]; i < offs[t + 1]; ++i) {
            const uint64_t gap = i == offs[t] ? (uint64_t)docs[i] + 1 : (uint64_t)(docs[i] - docs[i - 1]);
            cost += gap < small.size() ? small[gap] : order_logq(gap);
        }
    return cost;
}

// The twin. The inputs are checked (order_*_fault). doc_map: num_docs entries; trace: one count per (level, iteration) that ran.
inline void order_postings(uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs_in, order_params const& prm, unsigned threads,
                           std::vector<uint32_t>& doc_map, std::vector<uint64_t>& trace) {
    const uint64_t n = num_docs, total = offs[nlists];
    trace.clear();
    std::vector<uint32_t> order(n);
    for (uint64_t s = 0; s < n; ++s) order[s] = (uint32_t)s;
    if (order_level_runs(n, 0, prm)) {
        std::vector<uint32_t> logq(n + 3);
        order_log_table(n + 3, logq.data());
        std::vector<uint32_t> docs(docs_in, docs_in + total), payload(total, 0); // the lists in p0 order; the payload only travels
        std::vector<uint32_t> members(n), inv(n), half_of(n), next_order(n);
        std::vector<uint8_t> side(n);
        std::vector<uint64_t> gain(n);
        std::vector<int32_t> clamped(n);
        for (uint32_t level = 0; order_level_runs(n, level, prm); ++level) {
            if (level) remap_postings(n, nlists, offs, docs.data(), payload.data(), inv.data(), threads);
            for (uint64_t s = 0; s < n; ++s) {
                members[s] = (uint32_t)s;
                half_of[s] = order_segment_of(n, level + 1, s);
                side[s] = half_of[s] & 1u;
            }
            for (uint32_t it = 0; it < prm.iterations; ++it) {
                std::fill(gain.begin(), gain.end(), 0);
                for (uint64_t t = 0; t < nlists; ++t)
                    for (uint64_t i = offs[t]; i < offs[t + 1];) { // one run: the term's documents of one segment
                        const uint32_t seg = half_of[docs[i]] >> 1;
                        uint64_t j = i;
                        uint32_t deg[2] = {0, 0};
                        for (; j < offs[t + 1] && (half_of[docs[j]] >> 1) == seg; ++j) ++deg[side[docs[j]]];
                        const uint32_t size[2] = {(uint32_t)(order_bound(n, level + 1, 2ull * seg + 1) - order_bound(n, level + 1, 2ull * seg)),
                                                  (uint32_t)(order_bound(n, level + 1, 2ull * seg + 2) - order_bound(n, level + 1, 2ull * seg + 1))};
                        for (; i < j; ++i) {
                            const uint32_t a = side[docs[i]];
                            gain[docs[i]] += (uint64_t)order_term_cost(logq.data(), size[a], size[a ^ 1], deg[a], deg[a ^ 1]);
                        }
                    }
                for (uint64_t p = 0; p < n; ++p) clamped[p] = order_clamp_gain((int64_t)gain[p]);
                const uint64_t halves = 2ull << level;
                parallel_for(halves, threads, [&](uint64_t h, unsigned) {
                    std::sort(members.begin() + order_bound(n, level + 1, h), members.begin() + order_bound(n, level + 1, h + 1), [&](uint32_t x, uint32_t y) {
                        return clamped[x] != clamped[y] ? clamped[x] > clamped[y] : x < y;
                    });
                });
                uint64_t exchanges = 0;
                for (uint64_t k = 0; k < halves / 2; ++k) {
                    const uint64_t l0 = order_bound(n, level + 1, 2 * k), r0 = order_bound(n, level + 1, 2 * k + 1), r1 = order_bound(n, level + 1, 2 * k + 2);
                    const uint64_t m = std::min(r0 - l0, r1 - r0);
                    for (uint64_t i = 0; i < m; ++i) {
                        const uint32_t pl = members[l0 + i], pr = members[r0 + i];
                        if ((int64_t)clamped[pl] + (int64_t)clamped[pr] <= 0) continue;
                        std::swap(members[l0 + i], members[r0 + i]);
                        side[pl] = 1;
                        side[pr] = 0;
                        ++exchanges;
                    }
                }
                trace.push_back(exchanges);
                if (!exchanges) break;
            }
            for (uint64_t s = 0; s < n; ++s) {
                next_order[s] = order[members[s]];
                inv[members[s]] = (uint32_t)s;
            }
            order.swap(next_order);
        }
    }
    doc_map.resize(n);
    for (uint64_t s = 0; s < n; ++s) doc_map[order[s]] = (uint32_t)s;
}

} // namespace ds2i_host
