// invert_twin_check -- a stand-alone check of the host side of the inversion (ds2i_amd/csrc/host_invert.hpp: the checks and the two
// twins), meant to be compiled with -fsanitize=address,undefined and run on a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/invert_twin_check.cpp -o invert_twin_check
// The documents are made in closed form: 3000 documents of 0 to 69 tokens over 500 terms (an empty document first, last and in
// between; repeats; neighbours that end and begin with the same term; terms that never occur), and one document of 70 000 tokens, more
// than the twin's threshold for spreading the transposition over its workers. Their inversion must be what a count written out here
// gives, with 1, 3 and 16 threads; transposing it gives the canonical documents and transposing those gives it back; and every refusal
// names what the header says. Prints "OK" and returns 0, or says what differs and returns 1.
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../ds2i_amd/csrc/host_invert.hpp"

using namespace ds2i_host;

namespace {

constexpr uint32_t NUM_DOCS = 3001, NTERMS = 500;

int fail(std::string const& what) {
    std::printf("FAILED: %s\n", what.c_str());
    return 1;
}

void documents(std::vector<uint64_t>& offs, std::vector<uint32_t>& tokens) {
    offs.assign(1, 0);
    uint32_t x = 12345;
    auto next = [&] { return x = x * 1664525u + 1013904223u; };
    for (uint32_t d = 0; d < NUM_DOCS; ++d) {
        uint32_t n = d == 0 || d + 1 == NUM_DOCS || d % 97 == 5 ? 0 : next() % 70;
        if (d == 1500) n = 70000;
        for (uint32_t i = 0; i < n; ++i) tokens.push_back((next() >> 8) % 40 < 30 ? (next() >> 8) % 23 : 100 + (next() >> 8) % 390); // (terms 23 .. 99 and 490 .. 499 never occur)
        if (n && d % 3 == 0) tokens.back() = 7;
        if (n && d % 3 == 1) tokens[offs.back()] = 7; // (a document that ends with 7, then one that begins with it)
        offs.push_back(tokens.size());
    }
}

bool same(csr_matrix const& a, csr_matrix const& b) { return a.offs == b.offs && a.ids == b.ids && a.vals == b.vals; }

// what `run` throws, or ""
template <class Fn>
std::string thrown(Fn&& run) {
    try {
        run();
    } catch (std::exception const& e) {
        return e.what();
    }
    return "";
}

bool has(std::string const& s, const char* part) { return s.find(part) != std::string::npos; }

} // namespace

int main() {
    std::vector<uint64_t> offs;
    std::vector<uint32_t> tokens;
    documents(offs, tokens);
    if (!invert_shape_fault("check", NUM_DOCS, NTERMS, offs.data()).empty()) return fail("the offsets are refused");
    // the inversion written out: per term, a map from document to count, walked in order
    csr_matrix want;
    {
        std::vector<std::map<uint32_t, uint32_t>> per_term(NTERMS);
        for (uint32_t d = 0; d < NUM_DOCS; ++d)
            for (uint64_t i = offs[d]; i < offs[d + 1]; ++i) ++per_term[tokens[i]][d];
        want.offs.assign(1, 0);
        for (auto const& m : per_term) {
            for (auto const& kv : m) {
                want.ids.push_back(kv.first);
                want.vals.push_back(kv.second);
            }
            want.offs.push_back(want.ids.size());
        }
    }
    if (want.offs[8] - want.offs[7] < NUM_DOCS / 2 || want.offs[51] != want.offs[50]) return fail("the documents are not what they are meant to be");
    csr_matrix lists, fwd, back;
    std::vector<uint32_t> sizes;
    for (unsigned threads : {1u, 3u, 16u}) {
        invert_documents("check", NUM_DOCS, offs.data(), tokens.data(), NTERMS, threads, lists, sizes);
        if (!same(lists, want)) return fail("the inversion with " + std::to_string(threads) + " threads");
        for (uint32_t d = 0; d < NUM_DOCS; ++d)
            if (sizes[d] != offs[d + 1] - offs[d]) return fail("doc_sizes");
        check_columns("check", NTERMS, NUM_DOCS, lists.offs.data(), lists.ids.data(), threads);
        transpose_csr(NTERMS, NUM_DOCS, lists.offs.data(), lists.ids.data(), lists.vals.data(), threads, fwd);
        csr_matrix canon;
        canonical_documents(NUM_DOCS, offs.data(), tokens.data(), threads, canon);
        if (!same(fwd, canon)) return fail("the transposed lists are not the canonical documents");
        check_columns("check", NUM_DOCS, NTERMS, fwd.offs.data(), fwd.ids.data(), threads);
        transpose_csr(NUM_DOCS, NTERMS, fwd.offs.data(), fwd.ids.data(), fwd.vals.data(), threads, back);
        if (!same(back, lists)) return fail("transpose(transpose(x)) != x");
    }
    std::vector<uint32_t> term_map;
    std::vector<uint64_t> kept;
    nonempty_lists(NTERMS, lists.offs.data(), term_map, kept);
    if (term_map.size() + 1 != kept.size() || kept.back() != lists.ids.size() || term_map.size() >= NTERMS || term_map[23] != 100)
        return fail("nonempty_lists");
    // no documents, no terms, no tokens
    {
        const uint64_t none[1] = {0};
        const uint32_t nothing[1] = {0};
        invert_documents("check", 0, none, nothing, 0, 4, lists, sizes);
        if (lists.offs != std::vector<uint64_t>{0} || !lists.ids.empty() || !sizes.empty()) return fail("the empty collection");
        const uint64_t empty_docs[4] = {0, 0, 0, 0};
        invert_documents("check", 3, empty_docs, nothing, 2, 4, lists, sizes);
        if (lists.offs != std::vector<uint64_t>{0, 0, 0} || sizes != std::vector<uint32_t>{0, 0, 0}) return fail("three empty documents");
    }
    // the refusals, in the header's order
    {
        std::vector<uint64_t> bad = offs;
        bad[0] = 1;
        if (!has(invert_shape_fault("check", NUM_DOCS, 1ull << 32, bad.data()), "must start at 0")) return fail("offsets not from 0");
        bad = offs;
        std::swap(bad[10], bad[11]);
        if (!has(invert_shape_fault("check", NUM_DOCS, 1ull << 32, bad.data()), "doc_offsets decrease")) return fail("decreasing offsets");
        const uint64_t huge[3] = {0, 1ull << 32, (1ull << 32) + 1};
        if (!has(invert_shape_fault("check", 2, 1ull << 32, huge), "2^32 documents or terms")) return fail("2^32 terms come before the long document");
        if (!has(invert_shape_fault("check", 2, 5, huge), "row 0 of the documents holds 2^32 entries or more")) return fail("a document of 2^32 tokens");
        if (!has(transpose_shape_fault("check", 2, 1ull << 32, huge), "2^32 rows or columns")) return fail("2^32 columns");
        std::vector<uint32_t> t = tokens;
        t[offs[40] + 2] = NTERMS + 3;
        t[offs[900]] = NTERMS; // the first offender is named, whichever worker finds the other
        const std::string e = thrown([&] { invert_documents("check", NUM_DOCS, offs.data(), t.data(), NTERMS, 16, lists, sizes); });
        if (!has(e, "document 40 holds token 503 at position 2, outside the 500 terms")) return fail("a token outside the terms: " + e);
        invert_documents("check", NUM_DOCS, offs.data(), tokens.data(), NTERMS, 16, lists, sizes);
        std::vector<uint32_t> c = lists.ids;
        const uint64_t at = lists.offs[7] + 9;
        c[at] = c[at - 1];
        std::string e2 = thrown([&] { check_columns("check", NTERMS, NUM_DOCS, lists.offs.data(), c.data(), 16); });
        if (!has(e2, "the columns of row 7 do not strictly increase at position 9")) return fail("columns that do not increase: " + e2);
        c[lists.offs[3]] = NUM_DOCS;
        e2 = thrown([&] { check_columns("check", NTERMS, NUM_DOCS, lists.offs.data(), c.data(), 16); });
        if (!has(e2, "row 3 holds column 3001 at position 0, outside the 3001 columns")) return fail("a column outside: " + e2);
    }
    std::printf("OK\n");
    return 0;
}
