// merge_twin_check -- a stand-alone check of the host side of the merge (ds2i_amd/csrc/host_merge.hpp: the plan, its refusals and the
// twin), meant to be compiled with -fsanitize=address,undefined and run on a CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/merge_twin_check.cpp -o merge_twin_check
// The collection is the block edge shape in closed form: lists of 1, 2, 127, 128, 129, 256 and 257 postings, a run of 700 consecutive
// doc-ids and a list that ends with the last document, over 50 000 documents. It is cut into range shards (default doc maps, term maps
// for the terms a shard lacks) and round-robin shards (explicit doc maps); either merge must give the collection back. Prints "OK" and
// returns 0, or says what differs and returns 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../ds2i_amd/csrc/host_merge.hpp"

using namespace ds2i_host;

namespace {

struct list_t {
    std::vector<uint32_t> docs, freqs;
};
struct source_t {
    uint64_t num_docs = 0;
    std::vector<uint64_t> offs{0};
    std::vector<uint32_t> docs, freqs, doc_map, term_map;
    bool has_doc_map = false;
    void add(list_t const& l, uint32_t term) {
        docs.insert(docs.end(), l.docs.begin(), l.docs.end());
        freqs.insert(freqs.end(), l.freqs.begin(), l.freqs.end());
        offs.push_back(docs.size());
        term_map.push_back(term);
    }
    merge_shape shape() const {
        merge_shape m;
        m.num_docs = num_docs;
        m.nlists = offs.size() - 1;
        m.offs = offs.data();
        m.doc_map = has_doc_map ? doc_map.data() : nullptr;
        m.map_len = doc_map.size();
        m.term_map = term_map.data();
        m.terms_len = term_map.size();
        return m;
    }
};

constexpr uint32_t NUM_DOCS = 50000;

std::vector<list_t> collection() {
    std::vector<list_t> lists;
    const uint32_t lengths[] = {1, 2, 127, 128, 129, 256, 257};
    uint32_t k = 0;
    for (uint32_t m : lengths) {
        list_t l;
        const uint32_t stride = 2 * ((NUM_DOCS / 2 - 1) / m); // even doc-ids, spread over all documents
        for (uint32_t i = 0; i < m; ++i) {
            l.docs.push_back(2 * k + i * stride);
            l.freqs.push_back(1 + (i * 7 + k) % 39);
        }
        lists.push_back(l);
        ++k;
    }
    list_t run, end;
    for (uint32_t i = 0; i < 700; ++i) {
        run.docs.push_back(7000 + i);
        run.freqs.push_back(1 + i % 4);
    }
    for (uint32_t i = 0; i < 299; ++i) {
        end.docs.push_back(3 + 166 * i);
        end.freqs.push_back(1 + i % 39);
    }
    end.docs.push_back(NUM_DOCS - 1);
    end.freqs.push_back(5);
    lists.push_back(run);
    lists.push_back(end);
    return lists;
}

// shard s of k holds the documents `mine` says, renumbered by `local`; lists without a posting there are dropped
template <class Mine, class Local>
source_t shard(std::vector<list_t> const& lists, uint64_t num_docs, Mine mine, Local local) {
    source_t s;
    s.num_docs = num_docs;
    for (uint32_t t = 0; t < lists.size(); ++t) {
        list_t part;
        for (size_t i = 0; i < lists[t].docs.size(); ++i)
            if (mine(lists[t].docs[i])) {
                part.docs.push_back(local(lists[t].docs[i]));
                part.freqs.push_back(lists[t].freqs[i]);
            }
        if (!part.docs.empty()) s.add(part, t);
    }
    return s;
}

int fail(std::string const& what) {
    std::printf("FAILED: %s\n", what.c_str());
    return 1;
}

int check(const char* name, std::vector<source_t> const& sources, std::vector<list_t> const& want, bool identity, unsigned threads) {
    std::vector<merge_shape> shapes;
    std::vector<const uint32_t*> docs, freqs;
    for (source_t const& s : sources) {
        shapes.push_back(s.shape());
        docs.push_back(s.docs.data());
        freqs.push_back(s.freqs.data());
    }
    merge_plan plan;
    const std::string fault = merge_plan_fault("check", shapes.data(), (uint32_t)shapes.size(), 0, plan);
    if (!fault.empty()) return fail(std::string(name) + ": " + fault);
    if (plan.num_docs != NUM_DOCS || plan.nlists != want.size() || plan.identity != identity) return fail(std::string(name) + ": the plan's shape");
    std::vector<uint32_t> out_docs(plan.offs[plan.nlists]), out_freqs(plan.offs[plan.nlists]);
    merge_postings(shapes.data(), docs.data(), freqs.data(), (uint32_t)shapes.size(), plan, out_docs.data(), out_freqs.data(), threads);
    for (size_t t = 0; t < want.size(); ++t) {
        const uint64_t first = plan.offs[t], n = plan.offs[t + 1] - first;
        if (n != want[t].docs.size()) return fail(std::string(name) + ": length of list " + std::to_string(t));
        for (uint64_t i = 0; i < n; ++i)
            if (out_docs[first + i] != want[t].docs[i] || out_freqs[first + i] != want[t].freqs[i])
                return fail(std::string(name) + ": list " + std::to_string(t) + " position " + std::to_string(i));
    }
    return 0;
}

bool refused(std::vector<source_t> const& sources, uint64_t nlists, const char* words) {
    std::vector<merge_shape> shapes;
    for (source_t const& s : sources) shapes.push_back(s.shape());
    merge_plan plan;
    return merge_plan_fault("check", shapes.data(), (uint32_t)shapes.size(), nlists, plan).find(words) != std::string::npos;
}

} // namespace

int main() {
    const std::vector<list_t> lists = collection();
    for (unsigned threads : {1u, 3u, 16u}) {
        const uint32_t cuts[] = {0, 7300, 30001, NUM_DOCS};
        std::vector<source_t> ranges;
        for (int s = 0; s < 3; ++s) {
            const uint32_t lo = cuts[s], hi = cuts[s + 1];
            ranges.push_back(shard(lists, hi - lo, [=](uint32_t d) { return d >= lo && d < hi; }, [=](uint32_t d) { return d - lo; }));
        }
        if (check("range shards", ranges, lists, true, threads)) return 1;
        std::vector<source_t> robin;
        for (uint32_t s = 0; s < 3; ++s) {
            robin.push_back(shard(lists, (NUM_DOCS - s + 2) / 3, [=](uint32_t d) { return d % 3 == s; }, [](uint32_t d) { return d / 3; }));
            robin.back().has_doc_map = true;
            for (uint64_t i = 0; i < robin.back().num_docs; ++i) robin.back().doc_map.push_back((uint32_t)(3 * i + s));
        }
        if (check("round-robin shards", robin, lists, false, threads)) return 1;
        if (threads != 1) continue;
        // the refusals, each on a copy
        std::vector<source_t> bad = robin;
        bad[1].doc_map[4] = bad[0].doc_map[9];
        if (!refused(bad, 0, "which an earlier document took")) return fail("a doc-id taken twice is not refused");
        bad = robin;
        bad[2].doc_map.pop_back();
        if (!refused(bad, 0, "the doc map of source 2 holds")) return fail("a short doc map is not refused");
        bad = ranges;
        std::swap(bad[0].term_map[0], bad[0].term_map[1]);
        if (!refused(bad, 0, "does not increase")) return fail("a term map that decreases is not refused");
        if (!refused(ranges, lists.size() - 1, "outside the")) return fail("a term past the merged lists is not refused");
        const std::string no_list = "merged term " + std::to_string(lists.size()) + " receives no list: List must be nonempty";
        if (!refused(ranges, lists.size() + 2, no_list.c_str())) return fail("a term without a list is not refused");
        if (!refused({}, 0, "no source")) return fail("no source is not refused");
        // a doc-id past its source: the twin throws and reads nothing past a map
        bad = robin;
        bad[0].docs[0] = (uint32_t)bad[0].num_docs;
        std::vector<merge_shape> shapes;
        std::vector<const uint32_t*> docs, freqs;
        for (source_t const& s : bad) {
            shapes.push_back(s.shape());
            docs.push_back(s.docs.data());
            freqs.push_back(s.freqs.data());
        }
        merge_plan plan;
        if (!merge_plan_fault("check", shapes.data(), 3, 0, plan).empty()) return fail("the plan looks at no posting");
        std::vector<uint32_t> od(plan.offs[plan.nlists]), of(plan.offs[plan.nlists]);
        bool thrown = false;
        try {
            merge_postings(shapes.data(), docs.data(), freqs.data(), 3, plan, od.data(), of.data(), 2);
        } catch (std::exception const& e) {
            thrown = std::string(e.what()).find("outside the map") != std::string::npos;
        }
        if (!thrown) return fail("a doc-id outside its source is not refused");
    }
    std::printf("OK\n");
    return 0;
}
