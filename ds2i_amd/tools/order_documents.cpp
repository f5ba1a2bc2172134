// order_documents -- a document order for an index, computed on the GPU by recursive graph bisection: the step before
// convert_index --remap.
//
//   order_documents <type> <index> <out map> [--iterations N] [--min-half N] [--levels N] [--check] [--device <n>]
//
// <type> is any of the nine index types. Writes <out map>, one ds2i binary sequence [num_docs][num_docs x u32] with new doc-id =
// map[old doc-id] (the layout of a .sizes file): what convert_index --remap reads.
//   --iterations N   at most N iterations a level (default 20)
//   --min-half N     no half of fewer than N documents is made (default 16)
//   --levels N       at most N levels (default 32)
//   --check          the map is checked to be a permutation (ds2i_check_doc_map); then the index is extracted, renumbered on the host
//                    (ds2i_remap_postings) and the integer cost of its gaps (ds2i_postings_cost, 1/256 bits) printed before and after:
//                    "OK documents=<n> cost_before=<c> cost_after=<c>" on stdout, or "MISMATCH map ..." and exit code 1
//   --device <n>     the HIP device (default 0)
// A usage error and an unreadable index file are reported before any device is looked for. Flags may stand anywhere.
// Exit code: 0 success, 1 the map is not a permutation, 2 an error.
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <type> <index> <out map> [--iterations N] [--min-half N] [--levels N] [--check] [--device <n>]\n"
    "  writes <out map>: one binary sequence [num_docs][num_docs x u32], new doc-id = map[old doc-id], as convert_index --remap reads it\n";

// a blob freed on every path out
struct blob_t {
    ds2i_blob* b = nullptr;
    blob_t() {}
    blob_t(blob_t const&) = delete;
    blob_t& operator=(blob_t const&) = delete;
    ~blob_t() { ds2i_blob_free(b); }
    template <class T> const T* as() const { return (const T*)ds2i_blob_data(b); }
};

static bool number(const char* text, unsigned long max, uint32_t& out) {
    char* end = nullptr;
    const unsigned long v = std::strtoul(text, &end, 10);
    if (end == text || *end || text[0] == '-' || text[0] == '+' || v > max) return false;
    out = (uint32_t)v;
    return true;
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    bool check = false, bad_flag = false;
    uint32_t device = 0;
    ds2i_order_params params = {0, 0, 0};
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--check") check = true;
        else if (a == "--device" && i + 1 < argc) bad_flag |= !number(argv[++i], 1ul << 20, device);
        else if (a == "--iterations" && i + 1 < argc) bad_flag |= !number(argv[++i], 0xFFFFFFFFul, params.iterations);
        else if (a == "--min-half" && i + 1 < argc) bad_flag |= !number(argv[++i], 0xFFFFFFFFul, params.min_half);
        else if (a == "--levels" && i + 1 < argc) bad_flag |= !number(argv[++i], 0xFFFFFFFFul, params.max_levels);
        else if (a.rfind("--", 0) == 0) bad_flag = true;
        else pos.push_back(argv[i]);
    }
    if (bad_flag || pos.size() != 3) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    const int kind = tool::kind_of(pos[0]);
    if (kind < 0) {
        tool::logger(std::string("ERROR: Unknown type ") + pos[0]);
        return 2;
    }
    try {
        tool::mapped_file in(pos[1]);
        blob_t map, trace;
        double ms = 0.0;
        tool::hip_ok(ds2i_hip_order_index((int)device, kind, in.data, in.size, &params, &map.b, &trace.b, &ms), "ds2i_hip_order_index");
        const uint64_t num_docs = ds2i_blob_size(map.b) / 4, rounds = ds2i_blob_size(trace.b) / 8;
        {
            FILE* f = std::fopen(pos[2], "wb");
            if (!f) throw std::runtime_error(std::string("cannot write ") + pos[2]);
            const uint32_t len = (uint32_t)num_docs;
            const bool ok = std::fwrite(&len, 4, 1, f) == 1 && (!len || std::fwrite(map.as<uint32_t>(), 4, len, f) == len);
            if (std::fclose(f) || !ok) throw std::runtime_error(std::string("cannot write ") + pos[2]);
        }
        uint64_t exchanges = 0;
        for (uint64_t r = 0; r < rounds; ++r) exchanges += trace.as<uint64_t>()[r];
        std::ostringstream os;
        os << num_docs << " documents ordered in " << rounds << " iterations, " << exchanges << " exchanges, " << ms << " ms on the device";
        tool::logger(os.str());
        if (check) {
            if (ds2i_check_doc_map(map.as<uint32_t>(), num_docs) != 0) {
                std::cout << "MISMATCH map " << ds2i_hip_last_error() << std::endl;
                return 1;
            }
            uint64_t n = 0, lists = 0, before = 0, after = 0;
            blob_t offs, docs, freqs;
            tool::hip_ok(ds2i_hip_extract_collection((int)device, kind, in.data, in.size, &n, &lists, &offs.b, &docs.b, &freqs.b, nullptr),
                         "ds2i_hip_extract_collection");
            const uint64_t total = offs.as<uint64_t>()[lists];
            std::vector<uint32_t> d(docs.as<uint32_t>(), docs.as<uint32_t>() + total), f(freqs.as<uint32_t>(), freqs.as<uint32_t>() + total);
            if (d.empty()) d.push_back(0), f.push_back(0); // (pointers the library may check against NULL)
            tool::hip_ok(ds2i_postings_cost(lists, offs.as<uint64_t>(), d.data(), &before), "ds2i_postings_cost");
            tool::hip_ok(ds2i_remap_postings(n, lists, offs.as<uint64_t>(), d.data(), f.data(), map.as<uint32_t>(), 0), "ds2i_remap_postings");
            tool::hip_ok(ds2i_postings_cost(lists, offs.as<uint64_t>(), d.data(), &after), "ds2i_postings_cost");
            std::cout << "OK documents=" << num_docs << " cost_before=" << before << " cost_after=" << after << std::endl;
        }
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
