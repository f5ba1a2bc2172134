// shard_queries -- the `queries` driver over the shards split_index wrote: the shards answer the query log as one index, in the
// collection's doc-ids and with the collection's scores (ds2i_hip_shard_set_*).
//
//   shard_queries <index_type> <query_op[:query_op...]> <prefix> <nshards> [--k K] [--devices a,b,...] [--print] < query_log
//
// Reads, for every shard s < nshards, <prefix>.<s> (an index of <index_type>), <prefix>.<s>.docs and <prefix>.<s>.terms (the maps, one
// binary sequence [len][len x u32] each) and <prefix>.<s>.wand (split_index --wand; without it the shard answers `and` / `or` only). The
// collection is as large as the maps say: the largest doc-id and the largest term plus one. The statistics are the sums over the shards,
// which for a split with nothing deleted are the unsplit index's own.
//   --k K            the k of the ranked operators (default 10, at most 1024)
//   --devices a,b,.. shard s is opened on the (s mod the list's length)-th device of the list (default: 0)
//   --print          after the timing, one line per result on stdout: "<query> <rank> <doc-id> <score>", ranked operators only
// Query log and stats line as `queries`: one query per line, whitespace separated term ids; one JSON line per operator with type, query,
// avg, q50, q90, q95 (microseconds), qps, kernel_ms (the slowest shard's window plus the merge kernel) and shards. Batched: 1 untimed
// and 2 timed passes over the whole log; the quantiles come from at most 256 evenly spaced queries sent one per call.
// Exit code: 0 success, 2 an error (usage errors among them).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../include/ds2i_hip.hpp"
#include "tool_util.hpp"

using namespace ds2i_hip;

static const char* const USAGE = " <index_type> <query_op[:query_op...]> <prefix> <nshards> [--k K] [--devices a,b,...] [--print] < query_log\n";

// [len][len x u32], the length word counting exactly the words behind it
struct map_file {
    tool::mapped_file f;
    uint64_t len = 0;
    explicit map_file(std::string const& path) : f(path.c_str()) {
        uint32_t n = 0;
        if (f.size >= 4) std::memcpy(&n, f.data, 4);
        if (f.size < 4 || f.size != 4 * (uint64_t(n) + 1)) throw std::runtime_error("the map file " + path + " is no binary sequence");
        len = n;
    }
    const uint32_t* map() const { return (const uint32_t*)f.data + 1; }
};

static bool parse_list(const char* text, std::vector<int>& out) {
    for (const char* p = text;;) {
        char* end = nullptr;
        const long v = std::strtol(p, &end, 10);
        if (end == p || *p == '-' || *p == '+' || v > 1 << 20) return false;
        out.push_back((int)v);
        if (!*end) return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

static int op_of(std::string const& t) {
    static const char* names[] = {"and", "and_freq", "or", "or_freq", "ranked_and", "wand", "maxscore", "ranked_or"};
    for (int i = 0; i < 8; ++i)
        if (t == names[i]) return i;
    return -1;
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    bool bad = false, print = false;
    long k = 10, nshards = 0;
    std::vector<int> devices;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--print") print = true;
        else if (a == "--k" && i + 1 < argc) {
            char* end = nullptr;
            k = std::strtol(argv[++i], &end, 10);
            bad = bad || end == argv[i] || *end || k < 1 || k > DS2I_HIP_MAX_K_LONG;
        } else if (a == "--devices" && i + 1 < argc) bad = bad || !devices.empty() || !parse_list(argv[++i], devices);
        else if (a.rfind("--", 0) == 0) bad = true;
        else pos.push_back(argv[i]);
    }
    if (!bad && pos.size() == 4) {
        char* end = nullptr;
        nshards = std::strtol(pos[3], &end, 10);
        bad = end == pos[3] || *end || nshards < 1 || nshards > DS2I_HIP_MAX_SHARDS;
    }
    if (bad || pos.size() != 4) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    if (devices.empty()) devices.push_back(0);
    const std::string type = pos[0], prefix = pos[2];
    const int kind = tool::kind_of(type);
    if (kind < 0) {
        tool::logger("ERROR: Unknown type " + type);
        return 2;
    }
    std::vector<std::pair<std::string, int>> ops;
    {
        std::stringstream ss(pos[1]);
        std::string t;
        while (std::getline(ss, t, ':')) {
            const int op = op_of(t);
            if (op < 0 || op == DS2I_OP_AND_FREQ || op == DS2I_OP_OR_FREQ) {
                tool::logger("ERROR: Unsupported query type over shards: " + t);
                std::cerr << "usage: " << argv[0] << USAGE;
                return 2;
            }
            ops.emplace_back(t, op);
        }
    }
    try {
        std::vector<std::unique_ptr<tool::mapped_file>> images, wands;
        std::vector<std::unique_ptr<map_file>> docs, terms;
        std::vector<ds2i_shard_source> sources;
        uint64_t collection_docs = 0, collection_terms = 0;
        bool all_wand = true;
        for (long s = 0; s < nshards; ++s) {
            const std::string base = prefix + "." + std::to_string(s);
            images.emplace_back(new tool::mapped_file(base.c_str()));
            docs.emplace_back(new map_file(base + ".docs"));
            terms.emplace_back(new map_file(base + ".terms"));
            std::unique_ptr<tool::mapped_file> w;
            try {
                w.reset(new tool::mapped_file((base + ".wand").c_str()));
            } catch (std::exception const&) {
                all_wand = false;
            }
            wands.push_back(std::move(w));
            ds2i_shard_source src{};
            src.device = devices[(size_t)s % devices.size()];
            src.kind = kind;
            src.image = images.back()->data;
            src.bytes = images.back()->size;
            src.wand_image = wands.back() ? wands.back()->data : nullptr;
            src.wand_bytes = wands.back() ? wands.back()->size : 0;
            src.doc_map = docs.back()->map();
            src.map_len = docs.back()->len;
            src.term_map = terms.back()->map();
            src.terms_len = terms.back()->len;
            for (uint64_t i = 0; i < src.map_len; ++i) collection_docs = std::max<uint64_t>(collection_docs, (uint64_t)src.doc_map[i] + 1);
            for (uint64_t j = 0; j < src.terms_len; ++j) collection_terms = std::max<uint64_t>(collection_terms, (uint64_t)src.term_map[j] + 1);
            sources.push_back(src);
        }
        for (auto const& o : ops)
            if (o.second >= DS2I_OP_RANKED_AND && !all_wand) throw std::runtime_error(o.first + " needs " + prefix + ".<s>.wand for every shard (split_index --wand)");
        std::vector<term_id_vec> queries;
        std::string line;
        while (std::getline(std::cin, line)) {
            std::istringstream il(line);
            term_id_vec q;
            term_id_type t;
            while (il >> t) q.push_back(t);
            queries.push_back(q);
        }
        gpu_shard_set set(sources, collection_docs, collection_terms);
        tool::logger("Performing " + type + " queries on " + std::to_string(nshards) + " shard(s) of " + std::to_string(collection_docs) + " documents");
        for (auto const& o : ops) {
            tool::logger("Query type: " + o.first);
            if (queries.empty()) {
                tool::logger("---- " + type + " " + o.first + ": empty query log, nothing to do");
                continue;
            }
            const size_t runs = 2;
            double total = 0, kernel_ms = 0;
            gpu_shard_set::result last;
            for (size_t run = 0; run <= runs; ++run) {
                const double tick = tool::get_time_usecs();
                last = set(o.second, queries, (uint32_t)k);
                const double el = tool::get_time_usecs() - tick;
                if (run) {
                    total += el;
                    kernel_ms += *std::max_element(last.stats.kernel_ms, last.stats.kernel_ms + DS2I_HIP_MAX_SHARDS) + last.stats.merge_ms;
                }
            }
            const double avg = total / (runs * queries.size());
            std::vector<double> lat;
            const size_t step = std::max<size_t>(1, queries.size() / 256);
            for (size_t i = 0; i < queries.size(); i += step) {
                const double tick = tool::get_time_usecs();
                set(o.second, std::vector<term_id_vec>(1, queries[i]), (uint32_t)k);
                lat.push_back(tool::get_time_usecs() - tick);
            }
            std::sort(lat.begin(), lat.end());
            auto quantile = [&](size_t pct) { return lat[std::min(lat.size() - 1, pct * lat.size() / 100)]; };
            std::ostringstream os;
            os << "---- " << type << " " << o.first << "\nMean: " << avg << "\n50% quantile: " << quantile(50) << "\n90% quantile: " << quantile(90)
               << "\n95% quantile: " << quantile(95);
            tool::logger(os.str());
            std::printf("{\"type\": \"%s\", \"query\": \"%s\", \"avg\": %g, \"q50\": %g, \"q90\": %g, \"q95\": %g, \"qps\": %g, \"kernel_ms\": %g, "
                        "\"shards\": %ld}\n",
                        type.c_str(), o.first.c_str(), avg, quantile(50), quantile(90), quantile(95), 1e6 / avg, kernel_ms / runs, nshards);
            if (print && o.second >= DS2I_OP_RANKED_AND)
                for (size_t q = 0; q < queries.size(); ++q)
                    for (uint32_t i = 0; i < last.len[q]; ++i)
                        std::printf("%zu %u %u %.9g\n", q, i, last.docs[q * (size_t)k + i], (double)last.topk[q * (size_t)k + i]);
        }
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
