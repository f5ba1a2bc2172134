// split_twin_check -- a stand-alone check of the host side of the split (ds2i_amd/csrc/host_split.hpp: the checks, the tables and the
// twin), meant to be compiled with -fsanitize=address,undefined and run on a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/split_twin_check.cpp -o split_twin_check
// The collection is the block edge shape in closed form (the one of merge_twin_check.cpp): lists of 1, 2, 127, 128, 129, 256 and 257
// postings, a run of 700 consecutive doc-ids and a list that ends with the last document, over 50 000 documents, and an empty list. It
// is split by ranges, round robin and with every seventh document dropped; every shard must be what a filter written out here gives,
// and merging the shards of a split without drops (host_merge.hpp) must give the collection back. Prints "OK" and returns 0, or says
// what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../ds2i_amd/csrc/host_merge.hpp"
#include "../ds2i_amd/csrc/host_split.hpp"

using namespace ds2i_host;

namespace {

constexpr uint32_t NUM_DOCS = 50000;

struct csr_t {
    std::vector<uint64_t> offs{0};
    std::vector<uint32_t> docs, freqs;
    uint64_t nlists() const { return offs.size() - 1; }
    void end_list() { offs.push_back(docs.size()); }
};

csr_t collection() {
    csr_t c;
    const uint32_t lengths[] = {1, 2, 127, 128, 129, 256, 257};
    uint32_t k = 0;
    for (uint32_t m : lengths) {
        const uint32_t stride = 2 * ((NUM_DOCS / 2 - 1) / m); // even doc-ids, spread over all documents
        for (uint32_t i = 0; i < m; ++i) {
            c.docs.push_back(2 * k + i * stride);
            c.freqs.push_back(1 + (i * 7 + k) % 39);
        }
        c.end_list();
        ++k;
    }
    for (uint32_t i = 0; i < 700; ++i) {
        c.docs.push_back(7000 + i);
        c.freqs.push_back(1 + i % 4);
    }
    c.end_list();
    c.end_list(); // an empty list: it survives nowhere
    for (uint32_t i = 0; i < 299; ++i) {
        c.docs.push_back(3 + 166 * i);
        c.freqs.push_back(1 + i % 39);
    }
    c.docs.push_back(NUM_DOCS - 1);
    c.freqs.push_back(5);
    c.end_list();
    return c;
}

int fail(std::string const& what) {
    std::printf("FAILED: %s\n", what.c_str());
    return 1;
}

// every shard against a filter written out: documents counted in order, lists walked posting by posting
int check(const char* name, csr_t const& c, std::vector<uint32_t> const& shard_of, uint32_t nshards, unsigned threads, bool merge_back) {
    const std::string who = std::string(name) + ": ";
    if (!split_csr_fault("check", c.nlists(), c.offs.data()).empty()) return fail(who + "the offsets are refused");
    const std::string fault = split_assign_fault("check", NUM_DOCS, c.nlists(), shard_of.data(), nshards);
    if (!fault.empty()) return fail(who + fault);
    std::vector<split_shard> out;
    split_postings(NUM_DOCS, c.nlists(), c.offs.data(), c.docs.data(), c.freqs.data(), shard_of.data(), nshards, threads, out);
    if (out.size() != nshards) return fail(who + "the number of shards");
    for (uint32_t s = 0; s < nshards; ++s) {
        split_shard const& sh = out[s];
        std::vector<uint32_t> doc_map, local(NUM_DOCS, 0);
        for (uint32_t d = 0; d < NUM_DOCS; ++d)
            if (shard_of[d] == s) {
                local[d] = (uint32_t)doc_map.size();
                doc_map.push_back(d);
            }
        if (sh.num_docs != doc_map.size() || sh.doc_map != doc_map) return fail(who + "doc map of shard " + std::to_string(s));
        if (sh.offs.size() != sh.nlists + 1 || sh.term_map.size() != sh.nlists || sh.docs.size() != sh.offs.back() || sh.freqs.size() != sh.offs.back())
            return fail(who + "shape of shard " + std::to_string(s));
        uint64_t list = 0, at = 0;
        for (uint64_t t = 0; t < c.nlists(); ++t) {
            bool any = false;
            for (uint64_t i = c.offs[t]; i < c.offs[t + 1]; ++i) {
                if (shard_of[c.docs[i]] != s) continue;
                any = true;
                if (at >= sh.docs.size() || sh.docs[at] != local[c.docs[i]] || sh.freqs[at] != c.freqs[i])
                    return fail(who + "shard " + std::to_string(s) + " list " + std::to_string(t) + " posting " + std::to_string(i));
                ++at;
            }
            if (!any) continue;
            if (list >= sh.nlists || sh.term_map[list] != t || sh.offs[list + 1] != at) return fail(who + "term map of shard " + std::to_string(s));
            ++list;
        }
        if (list != sh.nlists || at != sh.docs.size()) return fail(who + "shard " + std::to_string(s) + " holds more than its postings");
    }
    if (!merge_back) return 0;
    // merge(split(x)) == x, but for the empty list, which no shard holds: it is left out of x too
    std::vector<merge_shape> shapes(nshards);
    std::vector<const uint32_t*> docs(nshards), freqs(nshards);
    for (uint32_t s = 0; s < nshards; ++s) {
        shapes[s].num_docs = out[s].num_docs;
        shapes[s].nlists = out[s].nlists;
        shapes[s].offs = out[s].offs.data();
        shapes[s].doc_map = out[s].doc_map.data();
        shapes[s].map_len = out[s].doc_map.size();
        shapes[s].term_map = out[s].term_map.data();
        shapes[s].terms_len = out[s].term_map.size();
        docs[s] = out[s].docs.data();
        freqs[s] = out[s].freqs.data();
    }
    merge_plan plan;
    const std::string refused = merge_plan_fault("check", shapes.data(), nshards, 0, plan);
    const uint64_t empty = 8; // the empty list's term
    if (refused.find("merged term " + std::to_string(empty) + " receives no list") == std::string::npos)
        return fail(who + "the merge does not name the empty list: " + refused);
    for (uint32_t s = 0; s < nshards; ++s)
        for (uint32_t& t : out[s].term_map)
            if (t > empty) --t;
    const std::string again = merge_plan_fault("check", shapes.data(), nshards, 0, plan);
    if (!again.empty()) return fail(who + again);
    if (plan.num_docs != NUM_DOCS || plan.nlists != c.nlists() - 1 || plan.offs[plan.nlists] != c.docs.size()) return fail(who + "the merged shape");
    std::vector<uint32_t> md(c.docs.size()), mf(c.docs.size());
    merge_postings(shapes.data(), docs.data(), freqs.data(), nshards, plan, md.data(), mf.data(), threads);
    if (md != c.docs || mf != c.freqs) return fail(who + "merging the shards does not give the collection back");
    return 0;
}

} // namespace

int main() {
    const csr_t c = collection();
    std::vector<uint32_t> ranges(NUM_DOCS), robin(NUM_DOCS), holes(NUM_DOCS), gone(NUM_DOCS, SPLIT_DROP), lonely(NUM_DOCS, 0);
    for (uint32_t d = 0; d < NUM_DOCS; ++d) {
        ranges[d] = d < 7300 ? 0 : d < 30001 ? 1 : 2;
        robin[d] = d % 3;
        holes[d] = d % 7 == 0 ? SPLIT_DROP : (d / 5) % 4;
    }
    lonely[1] = 1; // a shard of one document, which no list holds: it comes back without a list
    for (unsigned threads : {1u, 3u, 16u}) {
        if (check("range shards", c, ranges, 3, threads, true)) return 1;
        if (check("round-robin shards", c, robin, 3, threads, true)) return 1;
        if (check("one shard", c, std::vector<uint32_t>(NUM_DOCS, 0), 1, threads, true)) return 1;
        if (check("drops", c, holes, 4, threads, false)) return 1;
        if (check("a shard nobody is sent to", c, robin, 5, threads, false)) return 1;
        if (check("everything dropped", c, gone, 2, threads, false)) return 1;
        if (check("a shard without a posting", c, lonely, 2, threads, false)) return 1;
    }
    // the refusals
    if (split_assign_fault("check", NUM_DOCS, c.nlists(), robin.data(), 0).find("no shard") == std::string::npos) return fail("no shard is not refused");
    if (split_assign_fault("check", 1ull << 32, 1, robin.data(), 3).find("2^32") == std::string::npos) return fail("2^32 documents are not refused");
    // (2^32 lists: asked of the function itself, which reads no offsets; through the entry points the offsets, 32 GiB of them, come first)
    if (split_assign_fault("check", NUM_DOCS, 1ull << 32, robin.data(), 3).find("2^32") == std::string::npos) return fail("2^32 lists are not refused");
    if (!split_assign_fault("check", NUM_DOCS, (1ull << 32) - 1, robin.data(), 3).empty()) return fail("2^32 - 1 lists are refused");
    std::vector<uint32_t> bad = robin;
    bad[41] = 3;
    bad[77] = 9;
    if (split_assign_fault("check", NUM_DOCS, c.nlists(), bad.data(), 3).find("document 41 is sent to shard 3") == std::string::npos)
        return fail("the first document sent outside the shards is not named");
    bad[41] = SPLIT_DROP;
    if (split_assign_fault("check", NUM_DOCS, c.nlists(), bad.data(), 3).find("document 77 is sent to shard 9") == std::string::npos)
        return fail("the drop value is refused");
    csr_t down = c;
    std::swap(down.offs[2], down.offs[3]);
    if (split_csr_fault("check", down.nlists(), down.offs.data()).find("decrease") == std::string::npos) return fail("decreasing offsets are not refused");
    // a doc-id past the documents: the twin throws, reads nothing past shard_of and leaves `out` alone
    csr_t past = c;
    past.docs[past.offs[5]] = NUM_DOCS;
    std::vector<split_shard> out(1);
    out[0].num_docs = 77;
    bool thrown = false;
    try {
        split_postings(NUM_DOCS, past.nlists(), past.offs.data(), past.docs.data(), past.freqs.data(), robin.data(), 3, 2, out);
    } catch (std::exception const& e) {
        thrown = std::string(e.what()).find("outside the 50000 documents") != std::string::npos;
    }
    if (!thrown || out.size() != 1 || out[0].num_docs != 77) return fail("a doc-id outside the documents is not refused");
    std::printf("OK\n");
    return 0;
}
