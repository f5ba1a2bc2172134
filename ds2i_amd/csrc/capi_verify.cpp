// Host side of the index verification (include/ds2i_hip.h: ds2i_hip_index_verify, ds2i_hip_verify_collection): the argument
// checks, the structure comparison (number of documents, number of lists, list lengths -- on the host, before any device is
// touched), the staging of the expected postings in CSR form, ONE launch of k_verify_index[_side] (kernels_upload.inc) over every
// block of every list, and the report of the first difference. The kernel returns one word: the smallest (global posting index,
// doc-id before freq) that differs; the value the index holds there comes from the single-list decode of that one list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "capi_util.hpp"
#include "launchers.hpp"

namespace {

// seconds of {image parse + structure comparison, bare upload of the image, staging of the expected postings} of this thread's last
// call (ds2i_hip_verify_host_seconds)
thread_local double verify_host_s[3] = {0.0, 0.0, 0.0};
double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

int check_offsets(const char* who, uint64_t nlists, const uint64_t* offs) {
    if (offs[0] != 0) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": list_offsets must start at 0").c_str());
    for (uint64_t t = 0; t < nlists; ++t)
        if (offs[t + 1] < offs[t]) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": list_offsets decrease").c_str());
    return DS2I_OK;
}

// num_docs, the number of lists, then every list's length: true = a difference, and the report says which
bool structure_differs(uint64_t idx_num_docs, uint64_t idx_lists, const uint32_t* idx_len, uint64_t num_docs, uint64_t nlists,
                       const uint64_t* offs, ds2i_hip_verify_report* r) {
    if (idx_num_docs != num_docs) {
        r->what = DS2I_VERIFY_NUM_DOCS;
        r->got = idx_num_docs;
        r->expected = num_docs;
        return true;
    }
    if (idx_lists != nlists) {
        r->what = DS2I_VERIFY_LISTS;
        r->got = idx_lists;
        r->expected = nlists;
        return true;
    }
    for (uint64_t t = 0; t < nlists; ++t) {
        const uint64_t n = offs[t + 1] - offs[t];
        if (idx_len[t] != n) {
            r->what = DS2I_VERIFY_LENGTH;
            r->list = t;
            r->got = idx_len[t];
            r->expected = n;
            r->postings_checked = offs[t];
            return true;
        }
    }
    return false;
}

// the postings: the lengths agree list by list
int verify_postings(ds2i_hip_index* idx, const uint64_t* offs, const uint32_t* docs, const uint32_t* freqs, ds2i_hip_verify_report* r,
                    double* device_ms) {
    const uint64_t V = idx->size, total = offs[V];
    r->postings_checked = total;
    if (!V || !total || !idx->total_blocks) return DS2I_OK;
    const auto t0 = std::chrono::steady_clock::now();
    WalkStaging st("index verification", "the collection does not fit");
    int rc = st.stage(idx, 0, V, offs);
    if (rc != DS2I_OK) return rc;
    uint32_t *d_docs = nullptr, *d_freqs = nullptr;
    unsigned long long* d_bad = nullptr;
    if (st.dev.alloc(&d_docs, 4 * total) != hipSuccess || st.dev.alloc(&d_freqs, 4 * total) != hipSuccess || st.dev.alloc(&d_bad, 8) != hipSuccess) return st.nomem();
    unsigned long long key = ds2i_dev::VERIFY_NONE;
    HIP_OK(hipMemcpy(d_docs, docs, 4 * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_freqs, freqs, 4 * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_bad, &key, 8, hipMemcpyHostToDevice));
    verify_host_s[2] = seconds_since(t0);
    ds2i_dev::VerifyArgs a{};
    a.exp_docs = d_docs;
    a.exp_freqs = d_freqs;
    a.first_bad = d_bad;
    double ms = 0.0;
    rc = st.launch(idx, a, ds2i_launch_verify_index, ds2i_launch_verify_index_side, ms);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = ms;
    HIP_OK(hipMemcpy(&key, d_bad, 8, hipMemcpyDeviceToHost));
    if (key == ds2i_dev::VERIFY_NONE) return DS2I_OK;
    const uint64_t at = key >> 1;
    if (at >= total) return ds2i_set_error(DS2I_EDEVICE, "index verification: the kernel reported a posting outside the collection");
    const uint64_t t = (uint64_t)(std::upper_bound(offs, offs + V + 1, at) - offs) - 1; // (no list is empty: the lengths agree with the index's)
    r->what = (key & 1) ? DS2I_VERIFY_FREQ : DS2I_VERIFY_DOCID;
    r->list = t;
    r->position = at - offs[t];
    r->expected = (key & 1) ? freqs[at] : docs[at];
    r->postings_checked = at;
    // what the index holds there: the single-list decode of that one list (the same choice of decoder)
    std::vector<uint32_t> ld, lf;
    DS2I_TRY
    ld.resize(idx->list_n[t]);
    lf.resize(idx->list_n[t]);
    DS2I_CATCH
    uint64_t n = 0;
    rc = ds2i_hip_decode_list(idx, (uint32_t)t, ld.data(), lf.data(), ld.size(), &n);
    if (rc != DS2I_OK) return rc;
    r->got = (key & 1) ? lf[r->position] : ld[r->position];
    return DS2I_OK;
}

} // namespace

extern "C" {

int ds2i_hip_index_verify(ds2i_hip_index* idx, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                          const uint32_t* freqs, ds2i_hip_verify_report* report, double* device_ms) {
    if (!idx || !list_offsets || !docs || !freqs || !report) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_index_verify: null argument");
    const int rc = check_offsets("ds2i_hip_index_verify", nlists, list_offsets);
    if (rc != DS2I_OK) return rc;
    std::memset(report, 0, sizeof *report);
    if (device_ms) *device_ms = 0.0;
    verify_host_s[0] = verify_host_s[1] = verify_host_s[2] = 0.0;
    if (structure_differs(idx->num_docs, idx->size, idx->list_n.data(), num_docs, nlists, list_offsets, report)) return DS2I_OK;
    return verify_postings(idx, list_offsets, docs, freqs, report, device_ms);
}

int ds2i_hip_verify_collection(int device, int index_kind, const void* image, size_t bytes, uint64_t num_docs, uint64_t nlists,
                               const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs, ds2i_hip_verify_report* report,
                               double* device_ms) {
    if (!image || !list_offsets || !docs || !freqs || !report) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_verify_collection: null argument");
    if (index_kind < DS2I_BLOCK_OPTPFOR || index_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_verify_collection: unknown index kind");
    int rc = check_offsets("ds2i_hip_verify_collection", nlists, list_offsets);
    if (rc != DS2I_OK) return rc;
    // ---- the image on the host: its size, num_docs and every list's length
    verify_host_s[0] = verify_host_s[1] = verify_host_s[2] = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t img_docs = 0, img_lists = 0;
    std::vector<uint32_t> img_len;
    rc = ds2i_parse_image(index_kind, image, bytes, img_docs, img_lists, &img_len);
    if (rc != DS2I_OK) return rc;
    std::memset(report, 0, sizeof *report);
    if (device_ms) *device_ms = 0.0;
    const bool differs = structure_differs(img_docs, img_lists, img_len.data(), num_docs, nlists, list_offsets, report);
    verify_host_s[0] = seconds_since(t0);
    if (differs) return DS2I_OK;
    // ---- the device: a bare upload (no tables, no transcoding), the kernel, close
    rc = check_device("ds2i_hip_verify_collection", device);
    if (rc != DS2I_OK) return rc;
    ds2i_hip_index* raw = nullptr;
    const auto t1 = std::chrono::steady_clock::now();
    rc = ds2i_index_open_bare(device, index_kind, image, bytes, &raw);
    if (rc != DS2I_OK) return rc;
    IndexHandle idx(raw); // (closed on every path out, an exception's included)
    verify_host_s[1] = seconds_since(t1);
    return verify_postings(idx.get(), list_offsets, docs, freqs, report, device_ms);
}

void ds2i_hip_verify_host_seconds(double seconds[3]) {
    if (seconds) std::memcpy(seconds, verify_host_s, sizeof verify_host_s);
}

} // extern "C"
