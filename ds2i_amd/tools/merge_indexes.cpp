// merge_indexes -- index files of any kinds merged into one index file, on the GPU.
//
//   merge_indexes <to_type> <out_index> <type1> <in1> [--docs <map>] [--terms <map>] <type2> <in2> [--docs <map>] [--terms <map>] ...
//                 [--lists <n>] [--check] [--check-only] [--device <n>]
//
// Writes the image ds2i_hip_merge_indexes returns: byte-identical to what create_freq_index <to_type> writes for the merged
// collection. <typeN> is any index type; <to_type> one the GPU encoder writes (block_optpfor, block_varint, block_interpolative, opt,
// ef, single, uniform). --docs and --terms belong to the source named before them; each <map> is one ds2i binary sequence,
// [len][len x u32] (the layout of a .sizes file):
//   --docs <map>   merged doc-id = map[doc-id of the source]; without it the source's documents follow those of the sources before it.
//                  All documents of all sources must receive distinct ids that fill [0, the sum of the sources' documents).
//   --terms <map>  merged term = map[list of the source], strictly increasing; without it list t is term t.
//   --lists <n>    the merged number of lists (default: the smallest that holds every mapped term); every term must receive a list
// A map file that is missing, short or long is a usage error, found before any device is touched.
//   --check        every source is extracted (ds2i_hip_extract_collection), the extractions merged on the host (ds2i_merge_postings)
//                  and the written file verified against that (ds2i_hip_verify_collection): one line on stdout,
//                  "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." as create_freq_index --check prints it.
//   --check-only   nothing is merged or written: <out_index> as it stands is verified against the sources in that way
//   --device <n>   the HIP device (default 0)
// Flags may stand anywhere but --docs and --terms. Wand data is not merged: the normalised lengths divide by the average length of
// the merged collection, which the sources' wand files cannot give back; build it from the merged .sizes.
// Exit code: 0 success, 1 the written index does not match the sources, 2 an error.
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <to_type> <out_index> <type1> <in1> [--docs <map>] [--terms <map>] <type2> <in2> ... [--lists <n>] [--check] [--check-only] [--device <n>]\n"
    "  --docs / --terms belong to the source before them: <map> is one binary sequence [len][len x u32];\n"
    "  merged doc-id = docs map[doc-id] (default: after the earlier sources' documents), merged term = terms map[list] (default: the same)\n";

// one binary sequence whose length word counts exactly the words behind it
struct map_file {
    tool::mapped_file f;
    uint64_t len = 0;
    explicit map_file(const char* path) : f(path) {
        if (f.size < 4) throw std::runtime_error(std::string("the map file ") + path + " holds no length word");
        uint32_t n;
        std::memcpy(&n, f.data, 4);
        if (f.size != 4 * (uint64_t(n) + 1))
            throw std::runtime_error(std::string("the map file ") + path + " announces " + std::to_string(n) + " entries and holds " +
                                     std::to_string(f.size / 4 - 1) + " words");
        len = n;
    }
    const uint32_t* map() const { return (const uint32_t*)f.data + 1; }
};

struct source_arg {
    const char *type = nullptr, *path = nullptr, *docs = nullptr, *terms = nullptr;
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
};

static bool number(const char* text, long long max, long long& out) {
    char* end = nullptr;
    out = std::strtoll(text, &end, 10);
    return end != text && !*end && out >= 0 && out <= max;
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    std::vector<source_arg> args;
    bool check = false, check_only = false, bad = false;
    long long device = 0, lists = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--check") check = true;
        else if (a == "--check-only") check_only = true;
        else if ((a == "--docs" || a == "--terms") && i + 1 < argc) {
            // (the source is complete when an even number of words, at least four, stand before the flag)
            if (pos.size() < 4 || pos.size() % 2) bad = true;
            else {
                args.resize(pos.size() / 2 - 1);
                const char*& slot = a == "--docs" ? args.back().docs : args.back().terms;
                if (slot) bad = true;
                slot = argv[i + 1];
            }
            ++i;
        } else if (a == "--device" && i + 1 < argc) bad = !number(argv[++i], 1 << 20, device) || bad;
        else if (a == "--lists" && i + 1 < argc) bad = !number(argv[++i], 0xFFFFFFFFll, lists) || bad;
        else if (a.rfind("--", 0) == 0) bad = true;
        else pos.push_back(argv[i]);
    }
    if (bad || pos.size() < 4 || pos.size() % 2) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    args.resize(pos.size() / 2 - 1);
    const int to = tool::kind_of(pos[0]);
    if (to < 0) {
        tool::logger(std::string("ERROR: Unknown type ") + pos[0]);
        return 2;
    }
    const size_t nsrc = args.size();
    std::vector<int> kinds(nsrc);
    for (size_t s = 0; s < nsrc; ++s) {
        args[s].type = pos[2 + 2 * s];
        args[s].path = pos[3 + 2 * s];
        kinds[s] = tool::kind_of(args[s].type);
        if (kinds[s] < 0) {
            tool::logger(std::string("ERROR: Unknown type ") + args[s].type);
            return 2;
        }
    }
    try {
        std::vector<std::unique_ptr<map_file>> doc_maps(nsrc), term_maps(nsrc);
        try {
            for (size_t s = 0; s < nsrc; ++s) {
                if (args[s].docs) doc_maps[s].reset(new map_file(args[s].docs));
                if (args[s].terms) term_maps[s].reset(new map_file(args[s].terms));
            }
        } catch (std::exception const& e) {
            std::cerr << "ERROR: " << e.what() << "\nusage: " << argv[0] << USAGE;
            return 2;
        }
        std::vector<std::unique_ptr<tool::mapped_file>> in(nsrc);
        std::vector<ds2i_merge_source> src(nsrc);
        size_t in_bytes = 0;
        for (size_t s = 0; s < nsrc; ++s) {
            in[s].reset(new tool::mapped_file(args[s].path));
            in_bytes += in[s]->size;
            src[s].kind = kinds[s];
            src[s].image = in[s]->data;
            src[s].bytes = in[s]->size;
            src[s].doc_map = doc_maps[s] ? doc_maps[s]->map() : nullptr;
            src[s].map_len = doc_maps[s] ? doc_maps[s]->len : 0;
            src[s].term_map = term_maps[s] ? term_maps[s]->map() : nullptr;
            src[s].terms_len = term_maps[s] ? term_maps[s]->len : 0;
        }
        if (!check_only) {
            ds2i_blob* img = nullptr;
            tool::hip_ok(ds2i_hip_merge_indexes((int)device, src.data(), (uint32_t)nsrc, (uint64_t)lists, to, &img, nullptr), "ds2i_hip_merge_indexes");
            const size_t bytes = ds2i_blob_size(img);
            try {
                tool::write_blob(pos[1], img);
            } catch (...) {
                ds2i_blob_free(img);
                throw;
            }
            ds2i_blob_free(img);
            std::ostringstream os;
            os << in_bytes << " bytes of " << nsrc << " indexes -> " << bytes << " bytes of " << pos[0];
            tool::logger(os.str());
        }
        if (check || check_only) { // against the host twin over the extractions of the sources
            std::vector<std::unique_ptr<extracted>> c(nsrc);
            std::vector<ds2i_merge_postings_source> csr(nsrc);
            for (size_t s = 0; s < nsrc; ++s) {
                c[s].reset(new extracted((int)device, kinds[s], *in[s]));
                csr[s].num_docs = c[s]->num_docs;
                csr[s].nlists = c[s]->lists;
                csr[s].list_offsets = (const uint64_t*)ds2i_blob_data(c[s]->offsets);
                csr[s].docs = (const uint32_t*)ds2i_blob_data(c[s]->docs);
                csr[s].freqs = (const uint32_t*)ds2i_blob_data(c[s]->freqs);
                csr[s].doc_map = src[s].doc_map;
                csr[s].map_len = src[s].map_len;
                csr[s].term_map = src[s].term_map;
                csr[s].terms_len = src[s].terms_len;
            }
            uint64_t num_docs = 0, nlists = 0;
            ds2i_blob *mo = nullptr, *md = nullptr, *mf = nullptr;
            tool::hip_ok(ds2i_merge_postings(csr.data(), (uint32_t)nsrc, (uint64_t)lists, 0, &num_docs, &nlists, &mo, &md, &mf), "ds2i_merge_postings");
            c.clear();
            int rc = 2;
            try {
                rc = tool::check_index_file((int)device, to, pos[1], num_docs, nlists, (const uint64_t*)ds2i_blob_data(mo),
                                            (const uint32_t*)ds2i_blob_data(md), (const uint32_t*)ds2i_blob_data(mf));
            } catch (...) {
                ds2i_blob_free(mo);
                ds2i_blob_free(md);
                ds2i_blob_free(mf);
                throw;
            }
            ds2i_blob_free(mo);
            ds2i_blob_free(md);
            ds2i_blob_free(mf);
            return rc;
        }
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
