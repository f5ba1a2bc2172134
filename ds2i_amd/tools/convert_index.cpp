// convert_index -- an index file of one kind turned into an index file of another, or back into a collection, on the GPU.
//
//   convert_index <from_type> <in_index> <to_type> <out_index> [--check] [--device <n>]
//   convert_index <from_type> <in_index> <to_type> <out_index> --remap <map> [--wand <in.wand> <out.wand>] [--check] [--device <n>]
//   convert_index <from_type> <in_index> --dump <collection_basename> [--device <n>]
//
// The first form writes the image ds2i_hip_convert_index returns: byte-identical to what create_freq_index <to_type> writes for
// the collection the input was built from. <from_type> is any index type; <to_type> one the GPU encoder writes (block_optpfor,
// block_varint, block_interpolative, opt, ef, single, uniform).
//   --check       the input is extracted (ds2i_hip_extract_collection) and the written file verified against it
//                 (ds2i_hip_verify_collection): one line on stdout, "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." as
//                 create_freq_index --check prints it.
// The second form renumbers the documents on the way (ds2i_hip_remap_index): <map> is one ds2i binary sequence, [num_docs][num_docs x u32]
// (the layout of a .sizes file), new doc-id = map[old doc-id], a permutation. A map file that is missing, short or long is a usage
// error, found before any device is touched. The file written is what create_freq_index <to_type> writes for the renumbered collection.
//   --wand <in.wand> <out.wand>  the wand data renumbered too (ds2i_remap_wand): an index holds none
//   --check       the input is extracted, renumbered on the host (ds2i_remap_postings) and the written file verified against that
// The third form writes <basename>.docs and <basename>.freqs in the ds2i binary-collection form (little-endian u32 streams of
// [len][len x u32] sequences, .docs led by [1][num_docs]). No <basename>.sizes is written: an index does not hold the document
// sizes (nor wand data).
//   --device <n>  the HIP device (default 0)
// Flags may stand anywhere. Exit code: 0 success, 1 the written index does not match the input, 2 an error.
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <from_type> <in_index> <to_type> <out_index> [--remap <map> [--wand <in.wand> <out.wand>]] [--check] [--device <n>]\n"
    "       convert_index <from_type> <in_index> --dump <collection_basename> [--device <n>]\n"
    "  --dump writes <collection_basename>.docs and .freqs; no .sizes, because an index does not hold the document sizes\n"
    "  --remap renumbers the documents: <map> is one binary sequence [num_docs][num_docs x u32], new doc-id = map[old doc-id]\n";

// the doc-id map of --remap: one binary sequence whose length word counts exactly the words behind it
struct doc_map_file {
    tool::mapped_file f;
    uint64_t num_docs = 0;
    explicit doc_map_file(const char* path) : f(path) {
        if (f.size < 4) throw std::runtime_error(std::string("the map file ") + path + " holds no length word");
        uint32_t n;
        std::memcpy(&n, f.data, 4);
        if (f.size != 4 * (uint64_t(n) + 1))
            throw std::runtime_error(std::string("the map file ") + path + " announces " + std::to_string(n) + " documents and holds " +
                                     std::to_string(f.size / 4 - 1) + " words");
        num_docs = n;
    }
    const uint32_t* map() const { return (const uint32_t*)f.data + 1; }
};

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
    const char *map_path = nullptr, *wand_in = nullptr, *wand_out = nullptr;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--check") check = true;
        else if (a == "--dump") dump = true;
        else if (a == "--remap" && i + 1 < argc) map_path = argv[++i];
        else if (a == "--wand" && i + 2 < argc) {
            wand_in = argv[++i];
            wand_out = argv[++i];
        } else if (a == "--device" && i + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || v < 0 || v > 1 << 20) bad_flag = true; // (not a device number)
            device = (int)v;
        } else if (a.rfind("--", 0) == 0) bad_flag = true;
        else pos.push_back(argv[i]);
    }
    if (bad_flag || pos.size() != (dump ? 3u : 4u) || (dump && check) || (dump && map_path) || (wand_in && !map_path)) {
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
        std::unique_ptr<doc_map_file> map;
        if (map_path) {
            try {
                map.reset(new doc_map_file(map_path));
            } catch (std::exception const& e) {
                std::cerr << "ERROR: " << e.what() << "\nusage: " << argv[0] << USAGE;
                return 2;
            }
        }
        ds2i_blob* img = nullptr;
        if (map) tool::hip_ok(ds2i_hip_remap_index(device, from, in.data, in.size, map->map(), map->num_docs, to, &img, nullptr), "ds2i_hip_remap_index");
        else tool::hip_ok(ds2i_hip_convert_index(device, from, in.data, in.size, to, &img, nullptr), "ds2i_hip_convert_index");
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
        if (wand_in) {
            tool::mapped_file w(wand_in);
            ds2i_blob* wimg = nullptr;
            tool::hip_ok(ds2i_remap_wand(w.data, w.size, map->map(), map->num_docs, &wimg), "ds2i_remap_wand");
            try {
                tool::write_blob(wand_out, wimg);
            } catch (...) {
                ds2i_blob_free(wimg);
                throw;
            }
            ds2i_blob_free(wimg);
        }
        if (check && map) { // against the host twin over the extraction of the input
            extracted c(device, from, in);
            const uint64_t total = c.offs()[c.lists];
            std::vector<uint32_t> docs(c.d(), c.d() + total), freqs(c.f(), c.f() + total);
            tool::hip_ok(ds2i_remap_postings(c.num_docs, c.lists, c.offs(), docs.data(), freqs.data(), map->map(), 0), "ds2i_remap_postings");
            return tool::check_index_file(device, to, pos[3], c.num_docs, c.lists, c.offs(), docs.data(), freqs.data());
        }
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
