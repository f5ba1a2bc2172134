// what the tools that write index files share (create_freq_index, convert_index): writing a blob, and the verification of a written
// index file against a collection in CSR form with its one line on stdout
#pragma once
#include "../../include/ds2i_build.h"
#include "../../include/ds2i_hip.h"
#include "tool_util.hpp"

namespace tool {

inline void write_blob(const char* path, ds2i_blob* b) {
    FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error(std::string("cannot write ") + path);
    std::fwrite(ds2i_blob_data(b), 1, ds2i_blob_size(b), f);
    std::fclose(f);
}

inline void hip_ok(int rc, const char* what) {
    if (rc) throw std::runtime_error(std::string(what) + " failed: " + ds2i_hip_last_error());
}

// the index file against the collection: "OK lists=<V> postings=<n>" or "MISMATCH <what> ..." on stdout; returns the exit code
// (0: they match, 1: they do not); an error is thrown
inline int check_index_file(int device, int kind, const char* path, uint64_t num_docs, uint64_t lists, const uint64_t* offsets,
                            const uint32_t* docs, const uint32_t* freqs) {
    mapped_file img(path);
    ds2i_hip_verify_report r;
    hip_ok(ds2i_hip_verify_collection(device, kind, img.data, img.size, num_docs, lists, offsets, docs, freqs, &r, nullptr),
           "ds2i_hip_verify_collection");
    switch (r.what) {
    case DS2I_VERIFY_OK:
        std::cout << "OK lists=" << lists << " postings=" << r.postings_checked << std::endl;
        return 0;
    case DS2I_VERIFY_NUM_DOCS:
        std::cout << "MISMATCH num_docs got=" << r.got << " expected=" << r.expected << std::endl;
        return 1;
    case DS2I_VERIFY_LISTS:
        std::cout << "MISMATCH lists got=" << r.got << " expected=" << r.expected << std::endl;
        return 1;
    case DS2I_VERIFY_LENGTH:
        std::cout << "MISMATCH length list=" << r.list << " got=" << r.got << " expected=" << r.expected << std::endl;
        return 1;
    default:
        std::cout << "MISMATCH " << (r.what == DS2I_VERIFY_DOCID ? "docid" : "freq") << " list=" << r.list << " position=" << r.position
                  << " got=" << r.got << " expected=" << r.expected << " length=" << (offsets[r.list + 1] - offsets[r.list]) << std::endl;
        return 1;
    }
}

} // namespace tool
