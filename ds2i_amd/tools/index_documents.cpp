// index_documents -- documents (sequences of term ids, what a tokenizer emits) indexed on the GPU: the step before merge_indexes.
//
//   index_documents <type> <forward file> <nterms> <out index> [<out wand>] [--gpu-only|--check] [--device <n>]
//
// <forward file> is a ds2i binary collection with one sequence per document and no leading singleton: [n][n x u32], the n term ids of
// the document in any order, with repeats, each < <nterms>; n may be 0 (an empty document keeps its doc-id). <type> is one the GPU
// encoder writes (block_optpfor, block_varint, block_interpolative, opt, ef, single, uniform).
// Writes <out index> (the image ds2i_hip_invert_documents returns: byte-identical to what create_freq_index <type> writes for the
// inverted collection), <out index>.terms (the term id of every list of the image: terms that never occur get no list; one ds2i
// binary sequence [len][len x u32], as split_index writes it and merge_indexes --terms reads it), <out index>.sizes (one sequence of
// num_docs token counts, the ds2i .sizes format) and, when named, <out wand> (the wand data over those sizes).
//   --gpu-only       nothing but the device inversion runs (the default)
//   --check          the documents are inverted on the host too (ds2i_invert_documents) and the written index verified against that
//                    collection (ds2i_hip_verify_collection): "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." on stdout, as
//                    create_freq_index --check prints it
//   --device <n>     the HIP device (default 0)
// A usage error and an unreadable or truncated forward file are reported before any device is looked for. Flags may stand anywhere.
// Exit code: 0 success, 1 the written index does not match the documents, 2 an error.
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <type> <forward file> <nterms> <out index> [<out wand>] [--gpu-only|--check] [--device <n>]\n"
    "  <forward file>: one binary sequence [n][n x u32] of term ids < <nterms> per document, no leading singleton\n"
    "  writes <out index>, <out index>.terms and <out index>.sizes\n";

// a blob freed on every path out
struct blob_t {
    ds2i_blob* b = nullptr;
    blob_t() {}
    blob_t(blob_t const&) = delete;
    blob_t& operator=(blob_t const&) = delete;
    ~blob_t() { ds2i_blob_free(b); }
    template <class T> const T* as() const { return (const T*)ds2i_blob_data(b); }
    uint64_t words() const { return ds2i_blob_size(b) / 4; }
};

// one binary sequence: [len][len x u32]
static void write_sequence(std::string const& path, const uint32_t* v, uint64_t n) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    const uint32_t len = (uint32_t)n;
    const bool ok = std::fwrite(&len, 4, 1, f) == 1 && (!len || std::fwrite(v, 4, len, f) == len);
    if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + path);
}

// the documents of a forward file in CSR form; empty sequences are documents too
static void read_forward(tool::mapped_file const& f, std::vector<uint64_t>& offs, std::vector<uint32_t>& tokens) {
    if (f.size % 4) throw std::runtime_error("the forward file is not a sequence of 32-bit words");
    const uint32_t* w = (const uint32_t*)f.data;
    const uint64_t n = f.size / 4;
    offs.assign(1, 0);
    for (uint64_t pos = 0; pos < n;) {
        const uint64_t len = w[pos++];
        if (len > n - pos)
            throw std::runtime_error("the forward file is truncated: document " + std::to_string(offs.size() - 1) + " announces " + std::to_string(len) +
                                     " tokens and " + std::to_string(n - pos) + " words follow");
        tokens.insert(tokens.end(), w + pos, w + pos + len);
        offs.push_back(tokens.size());
        pos += len;
    }
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    bool check = false, gpu_only = false, bad_flag = false;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--check") check = true;
        else if (a == "--gpu-only") gpu_only = true;
        else if (a == "--device" && i + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || v < 0 || v > 1 << 20) bad_flag = true; // (not a device number)
            device = (int)v;
        } else if (a.rfind("--", 0) == 0) bad_flag = true;
        else pos.push_back(argv[i]);
    }
    unsigned long long nterms = 0;
    if (!bad_flag && pos.size() >= 3) {
        char* end = nullptr;
        nterms = std::strtoull(pos[2], &end, 10);
        if (end == pos[2] || *end || pos[2][0] == '-' || pos[2][0] == '+' || nterms > 0xFFFFFFFFull) bad_flag = true;
    }
    if (bad_flag || (check && gpu_only) || pos.size() < 4 || pos.size() > 5) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    const int kind = tool::kind_of(pos[0]);
    if (kind < 0) {
        tool::logger(std::string("ERROR: Unknown type ") + pos[0]);
        return 2;
    }
    try {
        std::vector<uint64_t> offs;
        std::vector<uint32_t> tokens;
        try {
            tool::mapped_file in(pos[1]);
            read_forward(in, offs, tokens);
        } catch (std::exception const& e) {
            std::cerr << "ERROR: " << e.what() << "\nusage: " << argv[0] << USAGE;
            return 2;
        }
        const uint64_t num_docs = offs.size() - 1;
        if (tokens.empty()) tokens.push_back(0); // (a pointer the library may check against NULL)
        blob_t image, wand, terms, sizes;
        double ms = 0.0;
        tool::hip_ok(ds2i_hip_invert_documents(device, kind, num_docs, offs.data(), tokens.data(), nterms, &image.b, pos.size() == 5 ? &wand.b : nullptr,
                                               &terms.b, &sizes.b, &ms),
                     "ds2i_hip_invert_documents");
        const std::string out = pos[3];
        tool::write_blob(out.c_str(), image.b);
        write_sequence(out + ".terms", terms.as<uint32_t>(), terms.words());
        write_sequence(out + ".sizes", sizes.as<uint32_t>(), sizes.words());
        if (pos.size() == 5) tool::write_blob(pos[4], wand.b);
        std::ostringstream os;
        os << num_docs << " documents, " << offs[num_docs] << " tokens -> " << terms.words() << " lists, " << ds2i_blob_size(image.b) << " bytes of "
           << pos[0] << ", " << ms << " ms on the device";
        tool::logger(os.str());
        if (check) { // against the host twin's nonempty lists
            blob_t lo, ld, lf, ls;
            tool::hip_ok(ds2i_invert_documents(num_docs, offs.data(), tokens.data(), nterms, 0, &lo.b, &ld.b, &lf.b, &ls.b), "ds2i_invert_documents");
            const uint64_t* all = lo.as<uint64_t>();
            std::vector<uint64_t> kept(1, 0);
            for (uint64_t t = 0; t < nterms; ++t)
                if (all[t + 1] != all[t]) kept.push_back(all[t + 1]);
            return tool::check_index_file(device, kind, out.c_str(), num_docs, kept.size() - 1, kept.data(), ld.as<uint32_t>(), lf.as<uint32_t>());
        }
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
