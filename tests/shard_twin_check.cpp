// shard_twin_check -- a stand-alone check of the host side of the shard set (ds2i_amd/csrc/host_shard.hpp: the merge of top-k rows with
// its argument checks, the wand data of a shard, the translation of a query), meant to be compiled with -fsanitize=address,undefined
// and run on a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/shard_twin_check.cpp -o shard_twin_check
// The merge runs over 1, 2, 3 and 64 row sets, k = 1, 2, 63, 64, 65, 256, 257 and 1024, 1 and 65 queries, rows of every length (empty,
// all empty, full), a handful of score values or a single one (the order then rests on the ids, which interleave across the row sets),
// no map, an increasing map, a permuted map and ids up to 0xFFFFFFFE; every output row must be what a comparison sort written out here
// gives -- by the float's value, then the id: no key is formed -- padded as the header says. The checks must name the first offender.
// split_wand must gather both arrays through maps that do not increase. Prints "OK" and returns 0, or says what differs and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../ds2i_amd/csrc/host_shard.hpp"

using namespace ds2i_host;

namespace {

[[noreturn]] void fail(const std::string& what) {
    std::printf("shard_twin_check: %s\n", what.c_str());
    std::exit(1);
}

uint64_t g_state = 0x5A4D5E7ull;
uint32_t rnd(uint32_t n) { // [0, n)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % (n ? n : 1));
}

struct RowSet {
    std::vector<float> scores;
    std::vector<uint32_t> docs, lens, map;
    bool has_map = false;
};

enum Fill { RANDOM, SOME_EMPTY, ALL_EMPTY, FULL };
enum Map { NONE, INCREASING, PERMUTED, HIGH };

// row set r of nrows: M local documents, the collection ids = r mod nrows; rows sorted by score descending, equal scores by local id
RowSet make(uint32_t r, uint32_t nrows, uint32_t nq, uint32_t k, Fill fill, bool equal, Map how) {
    static const float VALUES[] = {0.0f, 0.25f, 1.5f, 1.5000001f, 3.75f, 11.0f, 1e-30f};
    const uint32_t M = std::max(2 * k, 64u);
    const uint64_t base = how == HIGH ? 0xFFFFFFFEull - (uint64_t)M * nrows + 1 : 7;
    std::vector<uint32_t> coll(M);
    for (uint32_t l = 0; l < M; ++l) coll[l] = (uint32_t)(base + (uint64_t)l * nrows + r);
    if (how == PERMUTED)
        for (uint32_t l = M - 1; l > 0; --l) std::swap(coll[l], coll[rnd(l + 1)]);
    RowSet rs;
    rs.scores.assign((size_t)nq * k, -INFINITY);
    rs.docs.assign((size_t)nq * k, 0xFFFFFFFFu);
    rs.lens.assign(nq, 0);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t n = fill == RANDOM ? rnd(k + 1) : fill == SOME_EMPTY ? ((q + r) % 2 ? 0 : 1 + rnd(k)) : fill == ALL_EMPTY ? 0 : k;
        // n distinct local ids: a random start and stride 1 or 2 keep them inside M
        const uint32_t stride = n && 2 * n <= M ? 1 + rnd(2) : 1, first = rnd(M - stride * (n ? n - 1 : 0));
        std::vector<std::pair<float, uint32_t>> c;
        for (uint32_t i = 0; i < n; ++i) c.emplace_back(equal ? 2.5f : VALUES[rnd(7)], first + i * stride);
        if (how == HIGH && r == nrows - 1 && q == 0 && n) c.back().second = M - 1;
        std::stable_sort(c.begin(), c.end(), [](auto const& a, auto const& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
        rs.lens[q] = n;
        for (uint32_t i = 0; i < n; ++i) {
            rs.scores[(size_t)q * k + i] = c[i].first;
            rs.docs[(size_t)q * k + i] = how == NONE ? coll[c[i].second] : c[i].second;
        }
    }
    rs.has_map = how != NONE;
    if (rs.has_map) rs.map = coll;
    return rs;
}

std::vector<ds2i_topk_rows> views(const std::vector<RowSet>& sets) {
    std::vector<ds2i_topk_rows> v;
    for (const RowSet& s : sets) v.push_back(ds2i_topk_rows{s.scores.data(), s.docs.data(), s.lens.data(), s.has_map ? s.map.data() : nullptr, s.map.size()});
    return v;
}

unsigned long long g_cases = 0;

void merge_case(uint32_t nrows, uint32_t nq, uint32_t k, Fill fill, bool equal, Map how, unsigned threads) {
    const std::string where = std::to_string(nrows) + " row sets, k " + std::to_string(k) + ", " + std::to_string(nq) + " queries, fill " +
                              std::to_string(fill) + ", map " + std::to_string(how) + (equal ? ", equal scores" : "");
    std::vector<RowSet> sets;
    for (uint32_t r = 0; r < nrows; ++r) sets.push_back(make(r, nrows, nq, k, fill, equal, how));
    const std::vector<ds2i_topk_rows> rows = views(sets);
    const std::string fault = merge_topk_fault("check", rows.data(), nrows, nq, k, false);
    if (!fault.empty()) fail(where + ": valid rows are refused: " + fault);
    // (exactly nq * k and nq elements: one store past an end is the sanitizer's to find)
    std::vector<float> s((size_t)nq * k, 777.f);
    std::vector<uint32_t> d((size_t)nq * k, 777u), l(nq, 777u);
    merge_topk(rows.data(), nrows, nq, k, s.data(), d.data(), l.data(), threads);
    bool high_seen = false;
    for (uint32_t q = 0; q < nq; ++q) {
        std::vector<std::pair<float, uint32_t>> c;
        for (const RowSet& rs : sets)
            for (uint32_t i = 0; i < rs.lens[q]; ++i) {
                const uint32_t doc = rs.docs[(size_t)q * k + i];
                c.emplace_back(rs.scores[(size_t)q * k + i], rs.has_map ? rs.map[doc] : doc);
            }
        std::sort(c.begin(), c.end(), [](auto const& a, auto const& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
        const uint32_t n = (uint32_t)std::min<size_t>(k, c.size());
        if (l[q] != n) fail(where + ": length of query " + std::to_string(q));
        for (uint32_t i = 0; i < k; ++i) {
            const float ws = i < n ? c[i].first : -INFINITY;
            const uint32_t wd = i < n ? c[i].second : 0xFFFFFFFFu;
            if (float_bits(s[(size_t)q * k + i]) != float_bits(ws) || d[(size_t)q * k + i] != wd)
                fail(where + ": query " + std::to_string(q) + ", rank " + std::to_string(i) + ": doc " + std::to_string(d[(size_t)q * k + i]) + ", expected " +
                     std::to_string(wd));
            high_seen = high_seen || (i < n && wd == 0xFFFFFFFEu);
        }
    }
    if (how == HIGH && fill == FULL && nrows == 1 && !high_seen) fail(where + ": the id 0xFFFFFFFE never came back");
    ++g_cases;
}

void expect_fault(const std::string& what, const std::string& fault, const std::string& text) {
    if (fault.find(text) == std::string::npos) fail(what + ": \"" + fault + "\" does not say \"" + text + "\"");
}

void merge_checks() {
    const uint32_t k = 4, nq = 3;
    std::vector<RowSet> sets{make(0, 2, nq, k, FULL, false, INCREASING), make(1, 2, nq, k, FULL, false, INCREASING)};
    std::vector<ds2i_topk_rows> rows = views(sets);
    expect_fault("no rows", merge_topk_fault("m", nullptr, 2, nq, k, false), "null argument");
    expect_fault("no output", merge_topk_fault("m", rows.data(), 0, nq, 0, true), "null argument");
    expect_fault("no row set", merge_topk_fault("m", rows.data(), 0, nq, 0, false), "0 row sets");
    expect_fault("k = 0", merge_topk_fault("m", rows.data(), 2, nq, 0, false), "k = 0");
    expect_fault("k = 1025", merge_topk_fault("m", rows.data(), 2, nq, 1025, false), "k = 1025");
    sets[1].lens[2] = 5;
    sets[0].scores[0] = -1.f;
    sets[0].docs[0] = 100000;
    expect_fault("a length", merge_topk_fault("m", rows.data(), 2, nq, k, false), "row set 1, query 2: length 5");
    sets[1].lens[2] = 4;
    for (float bad : {-1.f, -0.f, INFINITY, NAN}) {
        sets[0].scores[0] = bad;
        expect_fault("a score", merge_topk_fault("m", rows.data(), 2, nq, k, false), "row set 0, query 0, position 0: the score");
    }
    sets[0].scores[0] = 11.f;
    expect_fault("an id", merge_topk_fault("m", rows.data(), 2, nq, k, false), "row set 0, query 0, position 0: local doc-id 100000");
    sets[0].docs[0] = 0;
    sets[0].lens[1] = 2; // what lies past a row's length is not looked at
    sets[0].scores[k + 2] = NAN;
    sets[0].docs[k + 3] = 100000;
    if (!merge_topk_fault("m", rows.data(), 2, nq, k, false).empty()) fail("entries past a row's length are looked at");
    // one collection id twice: both may come back, and nothing moves out of bounds
    std::vector<RowSet> twice{make(0, 1, 1, 2, FULL, true, NONE)};
    twice.push_back(twice[0]);
    twice.push_back(twice[0]);
    const std::vector<ds2i_topk_rows> tv = views(twice);
    std::vector<float> s(2);
    std::vector<uint32_t> d(2), l(1);
    merge_topk(tv.data(), 3, 1, 2, s.data(), d.data(), l.data(), 1);
    if (l[0] != 2 || d[0] != d[1]) fail("a repeated id");
}

void wand_checks() {
    const uint64_t N = 1000, V = 50;
    std::vector<float> nl(N), mw(V);
    for (uint64_t i = 0; i < N; ++i) nl[i] = 0.25f + (float)rnd(1000) / 256.f;
    for (uint64_t j = 0; j < V; ++j) mw[j] = 0.01f + (float)rnd(1000) / 1024.f;
    bytes_t image;
    wand_freeze(nl, mw, image);
    wand_view w;
    w.parse(image.data(), image.size());
    std::vector<uint32_t> dm, tm;
    for (uint32_t i = 0; i < 333; ++i) dm.push_back(rnd(N)); // neither increasing nor injective: a gather takes any map
    for (uint32_t j = 0; j < 20; ++j) tm.push_back(rnd(V));
    dm.push_back(N - 1);
    tm.push_back(V - 1);
    if (!split_wand_fault("w", w, dm.data(), dm.size(), tm.data(), tm.size()).empty()) fail("valid maps are refused");
    bytes_t out;
    split_wand(w, dm.data(), dm.size(), tm.data(), tm.size(), out);
    wand_view s;
    s.parse(out.data(), out.size());
    if (s.num_docs != dm.size() || s.num_terms != tm.size()) fail("the shape of the split wand data");
    for (size_t i = 0; i < dm.size(); ++i)
        if (std::memcmp(s.norm_lens + 4 * i, &nl[dm[i]], 4)) fail("norm_lens[" + std::to_string(i) + "]");
    for (size_t j = 0; j < tm.size(); ++j)
        if (std::memcmp(s.max_term_weight + 4 * j, &mw[tm[j]], 4)) fail("max_term_weight[" + std::to_string(j) + "]");
    bytes_t none;
    split_wand(w, nullptr, 0, nullptr, 0, none);
    if (none.size() != 16) fail("the wand data of nothing");
    dm[7] = N;
    dm[9] = N + 5;
    tm[3] = V;
    expect_fault("a document", split_wand_fault("w", w, dm.data(), dm.size(), tm.data(), tm.size()), "doc_map[7] = 1000");
    dm[7] = dm[9] = 0;
    expect_fault("a term", split_wand_fault("w", w, dm.data(), dm.size(), tm.data(), tm.size()), "term_map[3] = 50");
}

void translate_checks() {
    const uint32_t tm[] = {2, 5, 9};
    auto tr = [&](std::vector<uint32_t> q, bool conj, uint64_t nterms = 3) {
        std::vector<uint32_t> out{77};
        translate_query(q.data(), (uint32_t)q.size(), tm, nterms, conj, out);
        if (out[0] != 77) fail("translate_query touched what was there");
        return std::vector<uint32_t>(out.begin() + 1, out.end());
    };
    typedef std::vector<uint32_t> v;
    if (tr({5, 5, 2}, true) != v{1, 1, 0} || tr({5, 7}, true) != v{} || tr({5, 7}, false) != v{1} || tr({9, 2, 9, 3}, false) != v{2, 0, 2} ||
        tr({}, true) != v{} || tr({10, 0}, false) != v{} || tr({5}, false, 0) != v{} || tr({9}, true) != v{2})
        fail("translate_query");
}

} // namespace

int main() {
    const uint32_t ks[] = {1, 2, 63, 64, 65, 256, 257, 1024}, nrows_of[] = {1, 2, 3, 64};
    uint32_t turn = 0;
    for (uint32_t nrows : nrows_of)
        for (uint32_t k : ks) {
            const bool big = (uint64_t)nrows * k > 4096;
            for (Map how : {NONE, INCREASING, PERMUTED}) {
                merge_case(nrows, big ? 1 : 3, k, (Fill)(turn % 4 == 2 ? RANDOM : turn % 4), turn % 3 == 0, how, 1 + turn % 3);
                ++turn;
            }
            merge_case(nrows, big ? 1 : 2, k, FULL, true, big ? INCREASING : HIGH, 2);
        }
    merge_case(3, 65, 10, RANDOM, false, PERMUTED, 3);
    merge_case(2, 65, 65, SOME_EMPTY, false, INCREASING, 16);
    merge_case(3, 4, 64, ALL_EMPTY, false, INCREASING, 1);
    merge_case(3, 4, 64, FULL, true, INCREASING, 1);
    merge_case(3, 4, 64, FULL, true, PERMUTED, 1);
    merge_case(3, 4, 65, RANDOM, false, HIGH, 2);
    merge_checks();
    wand_checks();
    translate_checks();
    if (g_cases < 100) fail("too few cases ran");
    std::printf("OK\n");
    return 0;
}
