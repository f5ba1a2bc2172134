// create_freq_index / create_wand_data -- tools that turn a ds2i binary collection
// (<basename>.docs/.freqs/.sizes, reference README.md:152-174) into the on-disk images the query path loads.
// They stand in for the reference's create_freq_index.cpp:45-110 and create_wand_data.cpp:8-29, which cannot
// be built here (succinct/FastPFor/Boost absent).
//
//   create_freq_index <index_type> <collection_basename> <output_index> [<output_wand_data>] [--gpu] [--check] [--device <n>]
//   create_freq_index <index_type> <collection_basename> <existing_index> --check-only [--device <n>]
//
// Without flags everything runs on the CPU, one list at a time through ds2i_builder_*. Flags may follow the positional
// arguments in any order:
//   --gpu         the collection is read into one CSR and built on the GPU: ds2i_hip_build_collection when wand data is asked
//                 for, ds2i_hip_encode_index when it is not. The files are byte-identical to the CPU path's. block_qmx and
//                 block_mixed have no GPU encoder: exit code 2, nothing is written.
//   --check       after writing, the written index file is mapped again and verified against the collection on the GPU
//                 (ds2i_hip_verify_collection): every doc-id and freq of every list.
//   --check-only  nothing is built: an existing index file is verified against the collection.
//   --device <n>  the HIP device of --gpu / --check / --check-only (default 0)
// A verification prints one line on stdout, "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." with the fields that apply
// (list, position, got = what the index holds, expected = what the collection holds, length = the list's length).
// Exit code: 0 success, 1 the index does not match the collection, 2 an error (an unknown index type among them whenever a
// verification was asked for; without one it is logged and the exit code stays 0, as before).
#include "tool_verify.hpp"

#include <cstdlib>

static const char* const USAGE =
    " <index_type> <collection_basename> <output_index> [<output_wand_data>] [--gpu] [--check] [--device <n>]\n"
    "       create_freq_index <index_type> <collection_basename> <existing_index> --check-only [--device <n>]\n";

// the head of <base>.docs: one sequence of one element, the number of documents
static uint64_t read_num_docs(tool::binary_sequences& docs) {
    const uint32_t* d;
    size_t nd;
    if (!docs.next(d, nd) || nd != 1) throw std::invalid_argument("the .docs file must begin with a one-element sequence holding the number of documents");
    return d[0];
}

// the collection as one CSR: what the GPU entry points take
struct csr_collection {
    uint64_t num_docs = 0;
    std::vector<uint64_t> offsets{0};
    std::vector<uint32_t> docs, freqs;
    uint64_t lists() const { return offsets.size() - 1; }
    explicit csr_collection(std::string const& base) {
        tool::mapped_file fdocs((base + ".docs").c_str()), ffreqs((base + ".freqs").c_str());
        tool::binary_sequences ds(fdocs), fs(ffreqs);
        const uint32_t* d;
        const uint32_t* f;
        size_t nd, nf;
        num_docs = read_num_docs(ds);
        docs.reserve(fdocs.size / 4);
        freqs.reserve(ffreqs.size / 4);
        while (ds.next(d, nd)) {
            if (!fs.next(f, nf) || nf != nd) throw std::invalid_argument("docs/freqs sequences out of step");
            docs.insert(docs.end(), d, d + nd);
            freqs.insert(freqs.end(), f, f + nd);
            offsets.push_back(docs.size());
        }
        if (docs.empty()) { docs.push_back(0); freqs.push_back(0); } // (never read: the pointers must not be null)
    }
};

// the index file against the collection: the line on stdout, and the exit code
static int check_file(int device, int kind, const char* path, csr_collection const& c) {
    return tool::check_index_file(device, kind, path, c.num_docs, c.lists(), c.offsets.data(), c.docs.data(), c.freqs.data());
}

int main(int argc, const char** argv) {
    std::vector<const char*> pos;
    bool gpu = false, check = false, check_only = false, bad_flag = false;
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--gpu") gpu = true;
        else if (a == "--check") check = true;
        else if (a == "--check-only") check_only = true;
        else if (a == "--device" && i + 1 < argc) {
            char* end = nullptr;
            const long v = std::strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end || v < 0 || v > 1 << 20) bad_flag = true; // (not a device number)
            device = (int)v;
        } else if (a == "--device") bad_flag = true;
        else if (a.rfind("--", 0) == 0) bad_flag = true;
        else pos.push_back(argv[i]);
    }
    if (pos.size() < 3) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 1;
    }
    if (bad_flag || (check_only && (gpu || check || pos.size() > 3))) {
        std::cerr << "usage: " << argv[0] << USAGE;
        return 2;
    }
    const int kind = tool::kind_of(pos[0]);
    if (kind < 0) {
        tool::logger(std::string("ERROR: Unknown type ") + pos[0]);
        return (check || check_only) ? 2 : 0; // (a run that was asked to verify never reports success without verifying)
    }
    const char* const out_index = pos[2];
    const char* const out_wand = pos.size() > 3 ? pos[3] : nullptr;
    if (gpu && (kind == DS2I_BLOCK_QMX || kind == DS2I_BLOCK_MIXED)) {
        tool::logger(std::string("ERROR: ") + pos[0] + " has no GPU encoder; --gpu builds block_optpfor, block_varint, block_interpolative, "
                     "opt, ef, single and uniform (without --gpu every type is built on the CPU)");
        return 2;
    }
    try {
        const std::string base = pos[1];
        std::unique_ptr<csr_collection> csr;
        if (gpu || check || check_only) csr.reset(new csr_collection(base));
        if (check_only) return check_file(device, kind, out_index, *csr);
        if (gpu) {
            std::unique_ptr<tool::mapped_file> fsizes;
            const uint32_t* s = nullptr;
            if (out_wand) {
                fsizes.reset(new tool::mapped_file((base + ".sizes").c_str()));
                tool::binary_sequences sizes(*fsizes);
                size_t ns;
                if (!sizes.next(s, ns) || ns != csr->num_docs) throw std::invalid_argument("sizes file does not match num_docs");
            }
            ds2i_blob *img = nullptr, *wi = nullptr;
            if (out_wand)
                tool::hip_ok(ds2i_hip_build_collection(device, kind, s, csr->num_docs, csr->lists(), csr->offsets.data(), csr->docs.data(),
                                                       csr->freqs.data(), &img, &wi, nullptr), "ds2i_hip_build_collection");
            else
                tool::hip_ok(ds2i_hip_encode_index(device, kind, csr->num_docs, csr->lists(), csr->offsets.data(), csr->docs.data(),
                                                   csr->freqs.data(), &img, nullptr), "ds2i_hip_encode_index");
            tool::write_blob(out_index, img);
            std::ostringstream os;
            os << csr->lists() << " sequences, " << csr->offsets.back() << " postings, " << ds2i_blob_size(img) << " bytes ("
               << (8.0 * ds2i_blob_size(img) / csr->offsets.back()) << " bits/posting)";
            tool::logger(os.str());
            ds2i_blob_free(img);
            if (wi) {
                tool::write_blob(out_wand, wi);
                ds2i_blob_free(wi);
            }
            return check ? check_file(device, kind, out_index, *csr) : 0;
        }
        tool::mapped_file fdocs((base + ".docs").c_str()), ffreqs((base + ".freqs").c_str());
        tool::binary_sequences docs(fdocs), freqs(ffreqs);
        const uint32_t* d;
        const uint32_t* f;
        size_t nd, nf;
        const uint64_t num_docs = read_num_docs(docs);
        ds2i_builder* b = nullptr;
        if (ds2i_builder_create(kind, num_docs, &b)) throw std::runtime_error("ds2i_builder_create failed");
        ds2i_wand_builder* w = nullptr;
        std::unique_ptr<tool::mapped_file> fsizes;
        if (out_wand) {
            fsizes.reset(new tool::mapped_file((base + ".sizes").c_str()));
            tool::binary_sequences sizes(*fsizes);
            const uint32_t* s;
            size_t ns;
            if (!sizes.next(s, ns) || ns != num_docs) throw std::invalid_argument("sizes file does not match num_docs");
            if (ds2i_wand_create(s, num_docs, &w)) throw std::runtime_error("ds2i_wand_create failed");
        }
        size_t lists = 0, postings = 0;
        while (docs.next(d, nd)) {
            if (!freqs.next(f, nf) || nf != nd) throw std::invalid_argument("docs/freqs sequences out of step");
            if (ds2i_builder_add_posting_list(b, nd, d, f)) throw std::runtime_error("add_posting_list failed");
            if (w && ds2i_wand_add_list(w, nd, d, f)) throw std::runtime_error("wand_add_list failed");
            ++lists;
            postings += nd;
        }
        ds2i_blob* img = nullptr;
        if (ds2i_builder_freeze(b, &img)) throw std::runtime_error("freeze failed");
        tool::write_blob(out_index, img);
        std::ostringstream os;
        os << lists << " sequences, " << postings << " postings, " << ds2i_blob_size(img) << " bytes ("
           << (8.0 * ds2i_blob_size(img) / postings) << " bits/posting)";
        tool::logger(os.str());
        ds2i_blob_free(img);
        ds2i_builder_free(b);
        if (w) {
            ds2i_blob* wi = nullptr;
            if (ds2i_wand_freeze(w, &wi)) throw std::runtime_error("wand freeze failed");
            tool::write_blob(out_wand, wi);
            ds2i_blob_free(wi);
            ds2i_wand_free(w);
        }
        if (check) return check_file(device, kind, out_index, *csr);
    } catch (std::exception const& e) {
        tool::logger(std::string("ERROR: ") + e.what());
        return 2;
    }
    return 0;
}
