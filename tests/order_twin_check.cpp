// order_twin_check -- a stand-alone check of the host side of the document ordering (ds2i_amd/csrc/host_order.hpp: the checks, the
// logarithm table, the cost and the twin of recursive graph bisection), meant to be compiled with -fsanitize=address,undefined and run on
// a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/order_twin_check.cpp -o order_twin_check
// The collection is made in closed form: 1203 documents of 5 kinds in a scrambled order over 90 terms, with documents without a term,
// duplicated documents, a term in every document, a term in one and empty lists. The twin's map and trace must be those of a second
// statement of the algorithm written out here over a forward index (documents and their terms, degrees counted per document, no list
// ever sorted), with 1, 3 and 16 threads and with several parameter sets; the map must be a permutation and lower the cost; the clamp, the
// segment arithmetic and every refusal must be what the header says. Prints "OK" and returns 0, or says what differs and returns 1.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../ds2i_amd/csrc/host_order.hpp"

using namespace ds2i_host;

namespace {

constexpr uint32_t NUM_DOCS = 1203, NTERMS = 90;

int fail(std::string const& what) {
    std::printf("FAILED: %s\n", what.c_str());
    return 1;
}

// forward[d] = the terms of document d, increasing
void documents(std::vector<std::vector<uint32_t>>& forward) {
    forward.assign(NUM_DOCS, {});
    uint32_t x = 2463534242u;
    auto next = [&] { return (x = x * 1664525u + 1013904223u) >> 8; };
    for (uint32_t d = 0; d < NUM_DOCS; ++d) {
        if (d % 101 == 7) continue;                      // a document without a term
        if (d % 9 == 4 && d) { forward[d] = forward[d - 1]; continue; } // a copy of its left neighbour
        const uint32_t kind = next() % 5;
        std::vector<bool> has(NTERMS, false);
        for (uint32_t i = 0; i < 8; ++i) has[kind * 16 + next() % 16] = true;
        has[80 + next() % 6] = true;                     // terms 80 .. 85: shared by all kinds
        has[86] = true;                                  // a term in every document (that has any)
        if (d == 600) has[87] = true;                    // a term in one document; 88 and 89 never occur
        for (uint32_t t = 0; t < NTERMS; ++t)
            if (has[t]) forward[d].push_back(t);
    }
}

void invert(std::vector<std::vector<uint32_t>> const& forward, std::vector<uint64_t>& offs, std::vector<uint32_t>& docs) {
    std::vector<std::vector<uint32_t>> lists(NTERMS);
    for (uint32_t d = 0; d < forward.size(); ++d)
        for (uint32_t t : forward[d]) lists[t].push_back(d);
    offs.assign(1, 0);
    docs.clear();
    for (auto const& l : lists) {
        docs.insert(docs.end(), l.begin(), l.end());
        offs.push_back(docs.size());
    }
}

// the algorithm over the forward index: positions hold documents, degrees are counted per (term, half) by a pass over the documents
void reference(std::vector<std::vector<uint32_t>> const& forward, order_params const& prm, std::vector<uint32_t>& doc_map, std::vector<uint64_t>& trace) {
    const uint64_t n = forward.size();
    std::vector<uint32_t> logq(n + 3);
    for (uint64_t v = 0; v < n + 3; ++v) logq[v] = order_logq(v);
    std::vector<uint32_t> order(n);
    for (uint64_t s = 0; s < n; ++s) order[s] = (uint32_t)s;
    trace.clear();
    for (uint32_t level = 0; level < prm.max_levels && (n >> (level + 1)) >= prm.min_half; ++level) {
        const uint64_t halves = 2ull << level;
        std::vector<uint64_t> b(halves + 1);
        for (uint64_t h = 0; h <= halves; ++h) b[h] = (h * n) >> (level + 1);
        std::vector<uint32_t> at(order); // at[s]: the document in slot s now
        std::vector<uint32_t> start(n);  // start[doc]: its slot at the level's start (the tie rule's p0)
        for (uint64_t s = 0; s < n; ++s) start[order[s]] = (uint32_t)s;
        for (uint32_t it = 0; it < prm.iterations; ++it) {
            std::vector<std::vector<uint32_t>> deg(halves, std::vector<uint32_t>(NTERMS, 0));
            std::vector<int64_t> gain(n, 0);
            for (uint64_t h = 0; h < halves; ++h)
                for (uint64_t s = b[h]; s < b[h + 1]; ++s)
                    for (uint32_t t : forward[at[s]]) ++deg[h][t];
            for (uint64_t h = 0; h < halves; ++h)
                for (uint64_t s = b[h]; s < b[h + 1]; ++s) {
                    const uint64_t o = h ^ 1;
                    int64_t g = 0;
                    for (uint32_t t : forward[at[s]])
                        g += order_term_cost(logq.data(), (uint32_t)(b[h + 1] - b[h]), (uint32_t)(b[o + 1] - b[o]), deg[h][t], deg[o][t]);
                    gain[at[s]] = order_clamp_gain(g);
                }
            for (uint64_t h = 0; h < halves; ++h)
                std::sort(at.begin() + b[h], at.begin() + b[h + 1], [&](uint32_t x, uint32_t y) { return gain[x] != gain[y] ? gain[x] > gain[y] : start[x] < start[y]; });
            uint64_t exchanges = 0;
            for (uint64_t h = 0; h < halves; h += 2)
                for (uint64_t i = 0; i < std::min(b[h + 1] - b[h], b[h + 2] - b[h + 1]); ++i)
                    if (gain[at[b[h] + i]] + gain[at[b[h + 1] + i]] > 0) {
                        std::swap(at[b[h] + i], at[b[h + 1] + i]);
                        ++exchanges;
                    }
            trace.push_back(exchanges);
            if (!exchanges) break;
        }
        order = at;
    }
    doc_map.resize(n);
    for (uint64_t s = 0; s < n; ++s) doc_map[order[s]] = (uint32_t)s;
}

} // namespace

int main() {
    // the arithmetic
    if (order_logq(0) != 0 || order_logq(1) != 0 || order_logq(2) != 256 || order_logq(3) != 406 || order_logq(1u << 20) != 5120) return fail("order_logq");
    if (order_clamp_gain(INT64_MAX) != INT32_MAX || order_clamp_gain(INT64_MIN) != INT32_MIN || order_clamp_gain((int64_t)INT32_MAX + 1) != INT32_MAX ||
        order_clamp_gain((int64_t)INT32_MIN - 1) != INT32_MIN || order_clamp_gain(-5) != -5 || order_clamp_gain(INT32_MAX) != INT32_MAX ||
        order_clamp_gain(INT32_MIN) != INT32_MIN)
        return fail("order_clamp_gain");
    for (int64_t g : {(int64_t)INT32_MIN, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)INT32_MAX}) {
        if (order_key_gain(order_gain_key((int32_t)g)) != (int32_t)g) return fail("order_key_gain");
        if (g < INT32_MAX && order_gain_key((int32_t)g) <= order_gain_key((int32_t)(g + 1))) return fail("order_gain_key does not reverse the order");
    }
    for (uint64_t n : {1ull, 2ull, 77ull, 1203ull, 0xFFFFFFFDull})
        for (uint32_t level : {0u, 1u, 5u, 31u, 32u}) {
            if ((n >> level) == 0) continue;
            for (uint64_t k : {0ull, 1ull, (1ull << level) / 2, (1ull << level) - 1}) {
                if (k >= (1ull << level)) continue;
                const uint64_t lo = order_bound(n, level, k), hi = order_bound(n, level, k + 1);
                if (hi <= lo || hi > n) return fail("order_bound");
                if (order_segment_of(n, level, lo) != k || order_segment_of(n, level, hi - 1) != k) return fail("order_segment_of");
            }
        }
    // the refusals
    order_params prm;
    const uint64_t bad0[] = {1, 1}, dec[] = {0, 2, 1}, ok2[] = {0, 2, 3};
    const uint32_t d3[] = {1, 4, 0}, same[] = {3, 3, 0};
    if (order_offsets_fault("w", 1, bad0) != "w: list_offsets must start at 0" || order_offsets_fault("w", 2, dec) != "w: list_offsets decrease" ||
        !order_offsets_fault("w", 2, ok2).empty())
        return fail("order_offsets_fault");
    if (order_docs_fault("w", 4, 2, ok2, d3) != "w: list 0 holds doc-id 4, outside the 4 documents" || !order_docs_fault("w", 5, 2, ok2, d3).empty() ||
        order_docs_fault("w", 5, 2, ok2, same) != "w: the doc-ids of list 0 do not strictly increase at position 1")
        return fail("order_docs_fault");
    if (order_num_docs_fault("w", 0xFFFFFFFEull).empty() || !order_num_docs_fault("w", 0xFFFFFFFDull).empty()) return fail("order_num_docs_fault");
    if (order_params_fault("w", 65537, 0, 0, prm) != "w: iterations above 65536" || order_params_fault("w", 0, 0, 33, prm) != "w: max_levels above 32" ||
        !order_params_fault("w", 0, 0, 0, prm).empty() || prm.iterations != 20 || prm.min_half != 16 || prm.max_levels != 32 ||
        !order_params_fault("w", 3, 4, 5, prm).empty() || prm.iterations != 3 || prm.min_half != 4 || prm.max_levels != 5)
        return fail("order_params_fault");
    if (order_level_runs(31, 0, order_params()) || !order_level_runs(32, 0, order_params()) || order_level_runs(32, 1, order_params())) return fail("order_level_runs");

    // the twin against the statement over the forward index
    std::vector<std::vector<uint32_t>> forward;
    documents(forward);
    std::vector<uint64_t> offs;
    std::vector<uint32_t> docs;
    invert(forward, offs, docs);
    if (!order_docs_fault("w", NUM_DOCS, NTERMS, offs.data(), docs.data()).empty()) return fail("the collection is not one");
    const uint32_t sets[][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {3, 5, 4}, {20, 600, 32}, {20, 602, 32}};
    for (auto const& s : sets) {
        if (!order_params_fault("w", s[0], s[1], s[2], prm).empty()) return fail("parameters refused");
        std::vector<uint32_t> want_map, map;
        std::vector<uint64_t> want_trace, trace;
        reference(forward, prm, want_map, want_trace);
        for (unsigned threads : {1u, 3u, 16u}) {
            order_postings(NUM_DOCS, NTERMS, offs.data(), docs.data(), prm, threads, map, trace);
            const std::string at = " with parameters " + std::to_string(s[0]) + ", " + std::to_string(s[1]) + ", " + std::to_string(s[2]) + " on " + std::to_string(threads) + " threads";
            if (trace != want_trace) return fail("the trace differs" + at);
            if (map != want_map) return fail("the map differs" + at);
            if (!doc_map_fault(map.data(), NUM_DOCS).empty()) return fail("the map is no permutation" + at);
        }
        if (s[1] == 602 && (!trace.empty() || map[5] != 5 || map[NUM_DOCS - 1] != NUM_DOCS - 1)) return fail("fewer than 2 * min_half documents are not left alone");
        if (s[1] == 600 && trace.empty()) return fail("2 * min_half documents (and three more) run no level");
        if (s[0] == 0 && s[1] == 0 && s[2] == 0) { // the order is better
            std::vector<uint32_t> moved(docs), payload(docs.size(), 1);
            const uint64_t before = postings_cost(NTERMS, offs.data(), docs.data());
            remap_postings(NUM_DOCS, NTERMS, offs.data(), moved.data(), payload.data(), map.data(), 2);
            if (!order_docs_fault("w", NUM_DOCS, NTERMS, offs.data(), moved.data()).empty()) return fail("the remapped collection is not one");
            if (postings_cost(NTERMS, offs.data(), moved.data()) >= before) return fail("the order is not better");
        }
    }
    // no document, one document, no list
    {
        std::vector<uint32_t> map;
        std::vector<uint64_t> trace;
        const uint64_t none[] = {0};
        const uint32_t nothing[] = {0};
        order_postings(0, 0, none, nothing, order_params(), 1, map, trace);
        if (!map.empty() || !trace.empty()) return fail("no document");
        order_postings(1, 0, none, nothing, order_params(), 1, map, trace);
        if (map != std::vector<uint32_t>{0} || !trace.empty()) return fail("one document");
        order_postings(40, 0, none, nothing, order_params(), 1, map, trace);
        if (map.size() != 40 || map[39] != 39 || trace != std::vector<uint64_t>{0}) return fail("no list");
    }
    std::printf("OK\n");
    return 0;
}
