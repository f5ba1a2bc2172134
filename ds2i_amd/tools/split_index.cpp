// split_index -- an index file cut into shards by documents, or with documents deleted, on the GPU: the inverse of merge_indexes.
//
//   split_index <from_type> <in_index> <to_type> <out> (--assign <file> | --ranges c1,c2,...) [--wand <in.wand>] [--check] [--device <n>]
//
// Writes, for every shard s, <out>.<s> (the image ds2i_hip_split_index returns: byte-identical to what create_freq_index <to_type>
// writes for the shard's collection), <out>.<s>.docs (the old doc-id of every document of the shard) and <out>.<s>.terms (the old term
// of every list of the shard), the two maps as merge_indexes --docs / --terms reads them: one ds2i binary sequence, [len][len x u32].
// <from_type> is any index type; <to_type> one the GPU encoder writes (block_optpfor, block_varint, block_interpolative, opt, ef,
// single, uniform). The documents of a shard keep their order and are numbered from 0; a list with no posting in a shard is left out of
// it. Every shard must hold a document and receive a posting.
//   --assign <file>  one binary sequence [num_docs][num_docs x u32]: the shard of every document, or 4294967295 to delete it. The
//                    number of shards is the largest shard number plus one. A file that is missing, short or long is a usage error,
//                    found before any device is touched.
//   --ranges c1,c2,...  contiguous ranges of doc-ids: [0, c1), [c1, c2), ..., [cn, num_docs); strictly increasing, inside the index
//                    (the number of documents comes from the host parse of the input, ds2i_hip_image_shape: a cut outside it is
//                    found before any device is touched).
//   --check          the input is extracted (ds2i_hip_extract_collection), split on the host (ds2i_split_postings) and every written
//                    shard verified against that (ds2i_hip_verify_collection): one line per shard on stdout,
//                    "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." as create_freq_index --check prints it.
//   --wand <in.wand> the wand data of the input: <out>.<s>.wand is written beside every shard, the shard's wand data under the
//                    COLLECTION's normalisation (ds2i_split_wand: both arrays gathered through the shard's maps), which is what
//                    shard_queries opens the shard with. A file that is missing or is no wand data of the input is found before any
//                    device is touched.
//   --device <n>     the HIP device (default 0)
// When no document is deleted, the first line on stdout is the merge_indexes command line that puts the shards back together, into
// <out>.merged. Without --wand no wand data is written: the wand data of a shard as a collection of its own (normalised lengths divided by
// the shard's own average length) is built from the shard's document sizes, sizes[<out>.<s>.docs]. Flags may stand anywhere.
// Exit code: 0 success, 1 a written shard does not match the input, 2 an error.
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <from_type> <in_index> <to_type> <out> (--assign <file> | --ranges c1,c2,...) [--wand <in.wand>] [--check] [--device <n>]\n"
    "  --assign: <file> is one binary sequence [num_docs][num_docs x u32], the shard of every document (4294967295 deletes it)\n"
    "  --ranges: contiguous doc-id ranges [0, c1), [c1, c2), ..., [cn, num_docs)\n"
    "  --wand: <in.wand> is the input's wand data; <out>.<s>.wand is written under the collection's normalisation\n"
    "  writes <out>.<s>, <out>.<s>.docs and <out>.<s>.terms for every shard s\n";

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

// the shards of a split, freed on every path out
struct shards_t {
    ds2i_split_shard* s = nullptr;
    uint32_t n;
    explicit shards_t(uint32_t n_) : n(n_) {}
    shards_t(shards_t const&) = delete;
    shards_t& operator=(shards_t const&) = delete;
    ~shards_t() { ds2i_split_free(s, n); }
};

// "c1,c2,...": strictly increasing, positive
static bool parse_ranges(const char* text, std::vector<uint64_t>& cuts) {
    for (const char* p = text;;) {
        char* end = nullptr;
        const unsigned long long v = std::strtoull(p, &end, 10);
        if (end == p || *p == '-' || *p == '+' || v == 0 || v > 0xFFFFFFFFull || (!cuts.empty() && v <= cuts.back())) return false;
        cuts.push_back(v);
        if (!*end) return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

static void write_map(std::string const& path, ds2i_blob* b) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    const uint32_t len = (uint32_t)(ds2i_blob_size(b) / 4);
    const bool ok = std::fwrite(&len, 4, 1, f) == 1 && (!len || std::fwrite(ds2i_blob_data(b), 4, len, f) == len);
    if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + path);
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    bool check = false, bad_flag = false;
    const char *assign_path = nullptr, *ranges_text = nullptr, *wand_path = nullptr;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--check") check = true;
        else if (a == "--assign" && i + 1 < argc) {
            bad_flag = bad_flag || assign_path;
            assign_path = argv[++i];
        } else if (a == "--ranges" && i + 1 < argc) {
            bad_flag = bad_flag || ranges_text;
            ranges_text = argv[++i];
        } else if (a == "--wand" && i + 1 < argc) {
            bad_flag = bad_flag || wand_path;
            wand_path = argv[++i];
        } else if (a == "--device" && i + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || v < 0 || v > 1 << 20) bad_flag = true; // (not a device number)
            device = (int)v;
        } else if (a.rfind("--", 0) == 0) bad_flag = true;
        else pos.push_back(argv[i]);
    }
    std::vector<uint64_t> cuts;
    if (bad_flag || pos.size() != 4 || !assign_path == !ranges_text || (ranges_text && !parse_ranges(ranges_text, cuts))) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    const int from = tool::kind_of(pos[0]), to = tool::kind_of(pos[2]);
    if (from < 0 || to < 0) {
        tool::logger(std::string("ERROR: Unknown type ") + pos[from < 0 ? 0 : 2]);
        return 2;
    }
    try {
        std::unique_ptr<map_file> assign;
        if (assign_path) {
            try {
                assign.reset(new map_file(assign_path));
            } catch (std::exception const& e) {
                std::cerr << "ERROR: " << e.what() << "\nusage: " << argv[0] << USAGE;
                return 2;
            }
        }
        tool::mapped_file in(pos[1]);
        std::unique_ptr<tool::mapped_file> wand;
        if (wand_path) { // held against the input's shape on the host: no device yet
            try {
                wand.reset(new tool::mapped_file(wand_path));
            } catch (std::exception const& e) {
                std::cerr << "ERROR: " << e.what() << "\nusage: " << argv[0] << USAGE;
                return 2;
            }
            uint64_t num_docs = 0, lists = 0;
            tool::hip_ok(ds2i_hip_image_shape(from, in.data, in.size, &num_docs, &lists), "ds2i_hip_image_shape");
            ds2i_blob *nl = nullptr, *mw = nullptr;
            tool::hip_ok(ds2i_wand_arrays(wand->data, wand->size, &nl, &mw), "ds2i_wand_arrays");
            const uint64_t wdocs = ds2i_blob_size(nl) / 4, wterms = ds2i_blob_size(mw) / 4;
            ds2i_blob_free(nl);
            ds2i_blob_free(mw);
            if (wdocs != num_docs || wterms < lists)
                throw std::runtime_error("--wand: the wand data holds " + std::to_string(wdocs) + " documents and " + std::to_string(wterms) +
                                         " terms, the index " + std::to_string(num_docs) + " and " + std::to_string(lists));
        }
        std::unique_ptr<extracted> c;
        std::vector<uint32_t> ranged;
        const uint32_t* shard_of = nullptr;
        uint64_t map_len = 0;
        uint32_t nshards = 1;
        bool drops = false;
        if (assign) {
            shard_of = assign->map();
            map_len = assign->len;
            for (uint64_t d = 0; d < map_len; ++d) {
                if (shard_of[d] == DS2I_SPLIT_DROP) drops = true;
                else if (shard_of[d] >= nshards) nshards = shard_of[d] + 1;
            }
        } else {
            uint64_t num_docs = 0, lists = 0; // (from the host parse of the image: no device yet)
            tool::hip_ok(ds2i_hip_image_shape(from, in.data, in.size, &num_docs, &lists), "ds2i_hip_image_shape");
            if (cuts.back() >= num_docs) throw std::runtime_error("--ranges: " + std::to_string(cuts.back()) + " lies outside the " + std::to_string(num_docs) + " documents");
            ranged.resize(num_docs);
            nshards = (uint32_t)cuts.size() + 1;
            for (uint64_t d = 0, s = 0; d < num_docs; ++d) {
                while (s < cuts.size() && d >= cuts[s]) ++s;
                ranged[d] = (uint32_t)s;
            }
            shard_of = ranged.data();
            map_len = ranged.size();
        }
        shards_t got(nshards);
        tool::hip_ok(ds2i_hip_split_index(device, from, in.data, in.size, shard_of, map_len, nshards, to, &got.s, nullptr), "ds2i_hip_split_index");
        const std::string out = pos[3];
        size_t bytes = 0;
        std::ostringstream merge;
        merge << "merge_indexes " << pos[2] << " " << out << ".merged";
        for (uint32_t s = 0; s < nshards; ++s) {
            const std::string base = out + "." + std::to_string(s);
            tool::write_blob(base.c_str(), got.s[s].image);
            write_map(base + ".docs", got.s[s].doc_map);
            write_map(base + ".terms", got.s[s].term_map);
            if (wand) {
                ds2i_blob* w = nullptr;
                tool::hip_ok(ds2i_split_wand(wand->data, wand->size, (const uint32_t*)ds2i_blob_data(got.s[s].doc_map), ds2i_blob_size(got.s[s].doc_map) / 4,
                                             (const uint32_t*)ds2i_blob_data(got.s[s].term_map), ds2i_blob_size(got.s[s].term_map) / 4, &w),
                             "ds2i_split_wand");
                tool::write_blob((base + ".wand").c_str(), w);
                ds2i_blob_free(w);
            }
            bytes += ds2i_blob_size(got.s[s].image);
            merge << " " << pos[2] << " " << base << " --docs " << base << ".docs --terms " << base << ".terms";
        }
        std::ostringstream os;
        os << in.size << " bytes of " << pos[0] << " -> " << bytes << " bytes of " << pos[2] << " in " << nshards << " shards";
        tool::logger(os.str());
        if (!drops) std::cout << merge.str() << std::endl;
        else tool::logger("documents were deleted: the shards do not merge back into the input");
        if (check) { // against the host twin over the extraction of the input
            if (!c) c.reset(new extracted(device, from, in));
            shards_t want(nshards);
            tool::hip_ok(ds2i_split_postings(c->num_docs, c->lists, c->offs(), c->d(), c->f(), shard_of, nshards, 0, &want.s), "ds2i_split_postings");
            c.reset();
            int rc = 0;
            for (uint32_t s = 0; s < nshards; ++s) {
                const std::string base = out + "." + std::to_string(s);
                const ds2i_split_shard& w = want.s[s];
                if (tool::check_index_file(device, to, base.c_str(), w.num_docs, w.nlists, (const uint64_t*)ds2i_blob_data(w.list_offsets),
                                           (const uint32_t*)ds2i_blob_data(w.docs), (const uint32_t*)ds2i_blob_data(w.freqs)))
                    rc = 1;
            }
            return rc;
        }
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
