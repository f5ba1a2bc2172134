// convert_index -- an index file of one kind turned into an index file of another, or back into a collection, on the GPU.
//
//   convert_index <from_type> <in_index> <to_type> <out_index> [--check] [--device <n>]
//   convert_index <from_type> <in_index> --dump <collection_basename> [--device <n>]
//
// The first form writes the image ds2i_hip_convert_index returns: byte-identical to what create_freq_index <to_type> writes for
// the collection the input was built from. <from_type> is any index type; <to_type> one the GPU encoder writes (block_optpfor,
// block_varint, block_interpolative, opt, ef, single, uniform).
//   --check       the input is extracted (ds2i_hip_extract_collection) and the written file verified against it
//                 (ds2i_hip_verify_collection): one line on stdout, "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." as
//                 create_freq_index --check prints it.
// The second form writes <basename>.docs and <basename>.freqs in the ds2i binary-collection form (little-endian u32 streams of
// [len][len x u32] sequences, .docs led by [1][num_docs]). No <basename>.sizes is written: an index does not hold the document
// sizes (nor wand data).
//   --device <n>  the HIP device (default 0)
// Flags may stand anywhere. Exit code: 0 success, 1 the written index does not match the input, 2 an error.
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <from_type> <in_index> <to_type> <out_index> [--check] [--device <n>]\n"
    "       convert_index <from_type> <in_index> --dump <collection_basename> [--device <n>]\n"
    "  --dump writes <collection_basename>.docs and .freqs; no .sizes, because an index does not hold the document sizes\n";

// the collection an index file holds
struct extracted {
    uint64_t num_docs = 0, lists = 0;
    ds2i_blob *offsets = nullptr, *docs = nullptr, *freqs = nullptr;
    extracted(int device, int kind, tool::mapped_file const& img) {
        tool::hip_ok(ds2i_hip_extract_collection(device, kind, img.data, img.size, &num_docs, &lists, &offsets, &docs, &freqs, nullptr),
                     "ds2i_hip_extract_collection");
    }
    extracted(extracted const&) = delete;
    extracted& operator=(extracted const&) = delete;
    ~extracted() {
        ds2i_blob_free(offsets);
        ds2i_blob_free(docs);
        ds2i_blob_free(freqs);
    }
    const uint64_t* offs() const { return (const uint64_t*)ds2i_blob_data(offsets); }
    const uint32_t* d() const { return (const uint32_t*)ds2i_blob_data(docs); }
    const uint32_t* f() const { return (const uint32_t*)ds2i_blob_data(freqs); }
};

static void write_words(FILE* f, const uint32_t* w, size_t n, const char* path) {
    if (n && std::fwrite(w, 4, n, f) != n) throw std::runtime_error(std::string("cannot write ") + path);
}

// one file of the binary collection: every list as [len][len x u32], behind `head`
static void write_sequences(std::string const& path, std::vector<uint32_t> const& head, extracted const& c, const uint32_t* values) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    try {
        write_words(f, head.data(), head.size(), path.c_str());
        for (uint64_t t = 0; t < c.lists; ++t) {
            const uint64_t n = c.offs()[t + 1] - c.offs()[t];
            const uint32_t len = (uint32_t)n;
            write_words(f, &len, 1, path.c_str());
            write_words(f, values + c.offs()[t], n, path.c_str());
        }
    } catch (...) {
        std::fclose(f);
        throw;
    }
    if (std::fclose(f)) throw std::runtime_error("cannot write " + path);
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    bool check = false, dump = false, bad_flag = false;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--check") check = true;
        else if (a == "--dump") dump = true;
        else if (a == "--device" && i + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || v < 0 || v > 1 << 20) bad_flag = true; // (not a device number)
            device = (int)v;
        } else if (a.rfind("--", 0) == 0) bad_flag = true;
        else pos.push_back(argv[i]);
    }
    if (bad_flag || pos.size() != (dump ? 3u : 4u) || (dump && check)) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    const int from = tool::kind_of(pos[0]);
    if (from < 0) {
        tool::logger(std::string("ERROR: Unknown type ") + pos[0]);
        return 2;
    }
    try {
        tool::mapped_file in(pos[1]);
        if (dump) {
            const std::string base = pos[2];
            extracted c(device, from, in);
            if (c.num_docs > 0xFFFFFFFFull) throw std::runtime_error("the number of documents does not fit the collection's 32-bit head");
            write_sequences(base + ".docs", {1u, (uint32_t)c.num_docs}, c, c.d());
            write_sequences(base + ".freqs", {}, c, c.f());
            std::ostringstream os;
            os << c.lists << " sequences, " << c.offs()[c.lists] << " postings";
            tool::logger(os.str());
            return 0;
        }
        const int to = tool::kind_of(pos[2]);
        if (to < 0) {
            tool::logger(std::string("ERROR: Unknown type ") + pos[2]);
            return 2;
        }
        ds2i_blob* img = nullptr;
        tool::hip_ok(ds2i_hip_convert_index(device, from, in.data, in.size, to, &img, nullptr), "ds2i_hip_convert_index");
        const size_t bytes = ds2i_blob_size(img);
        try {
            tool::write_blob(pos[3], img);
        } catch (...) {
            ds2i_blob_free(img);
            throw;
        }
        ds2i_blob_free(img);
        std::ostringstream os;
        os << in.size << " bytes of " << pos[0] << " -> " << bytes << " bytes of " << pos[2];
        tool::logger(os.str());
        if (check) {
            extracted c(device, from, in);
            return tool::check_index_file(device, to, pos[3], c.num_docs, c.lists, c.offs(), c.d(), c.f());
        }
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
