// Host side of the extraction (include/ds2i_hip.h: ds2i_hip_index_extract, ds2i_hip_extract_collection, ds2i_hip_convert_index): the
// argument checks, the host parse of an image before any device is touched, ONE launch of k_extract_index[_side]
// (kernels_upload.inc: the verifier's whole-index walk with stores instead of compares) over the blocks of a range of lists, and
// what is done with the postings: copied to the caller, or handed to the index encoder where they lie (capi_encode.cpp,
// ds2i_encode_device_postings), so that a conversion between kinds never sends them over the bus -- renumbered on the way through a doc-id map when one is given
// (capi_remap.cpp: ds2i_remap_device_postings, the step ds2i_hip_remap_index adds to a conversion). The host parse, the extraction
// into device buffers and the conversion of an image are declared in capi_util.hpp: the verification and the transcoding upload
// (capi.cpp, index_open_transcoded) use them too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "capi_blob.hpp"
#include "capi_util.hpp"
#include "host_index.hpp"
#include "host_pef.hpp"
#include "launchers.hpp"

namespace {

// seconds of {image parse, bare upload of the image, copy of the postings to the host} of this thread's last
// ds2i_hip_extract_collection (ds2i_hip_extract_host_seconds)
thread_local double extract_host_s[3] = {0.0, 0.0, 0.0};
double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// offs[0 .. end - begin] = where every list of [begin, end) starts in the output, from 0
void range_offsets(const ds2i_hip_index* idx, uint64_t begin, uint64_t end, uint64_t* offs) {
    offs[0] = 0;
    for (uint64_t t = begin; t < end; ++t) offs[t - begin + 1] = offs[t - begin] + idx->list_n[t];
}

} // namespace

int ds2i_parse_image(int index_kind, const void* image, size_t bytes, uint64_t& num_docs, uint64_t& nlists, std::vector<uint32_t>* lengths) {
    DS2I_TRY
    if (ds2i_host::is_freq_layout(index_kind)) {
        ds2i_host::opt_index_view v;
        v.layout = index_kind;
        v.parse(image, bytes);
        num_docs = v.num_docs;
        nlists = v.size;
        if (lengths) {
            lengths->resize(v.size);
            for (uint64_t t = 0; t < v.size; ++t) (*lengths)[t] = (uint32_t)v.list_length(t);
        }
    } else {
        ds2i_host::block_index_view v;
        v.parse(image, bytes);
        num_docs = v.num_docs;
        nlists = v.size;
        if (lengths) lengths->resize(v.size);
        for (uint64_t t = 0; t < v.size; ++t) {
            uint32_t n = 0;
            if (!ds2i_host_vbyte(v.lists + v.list_offsets[t], v.list_offsets[t + 1] - v.list_offsets[t], n) || !n)
                return ds2i_set_error(DS2I_EFORMAT, "posting list header is corrupt");
            if (lengths) (*lengths)[t] = n;
        }
    }
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_extract_to_device(ds2i_hip_index* idx, uint64_t begin, uint64_t end, const uint64_t* offs, DevPostings& out, double& ms) {
    const uint64_t total = offs[end - begin];
    WalkStaging st("index extraction", "the postings do not fit");
    int rc = st.stage(idx, begin, end, offs);
    if (rc != DS2I_OK) return rc;
    // (hipMalloc of 0 bytes gives no pointer to free: the buffers of an empty range hold one unused word)
    if (hipMalloc((void**)&out.docs, 4 * std::max<uint64_t>(total, 1)) != hipSuccess || hipMalloc((void**)&out.freqs, 4 * std::max<uint64_t>(total, 1)) != hipSuccess)
        return st.nomem();
    ds2i_dev::ExtractArgs a{};
    a.out_docs = out.docs;
    a.out_freqs = out.freqs;
    return st.launch(idx, a, ds2i_launch_extract_index, ds2i_launch_extract_index_side, ms);
}

int ds2i_convert_image(const char* who, int device, int from_kind, const void* image, size_t bytes, int to_kind, ds2i_blob** out_image, double* device_ms,
                       bool* no_room, const uint32_t* doc_map, double* remap_ms) {
    ds2i_hip_index* raw = nullptr;
    int rc = ds2i_index_open_bare(device, from_kind, image, bytes, &raw);
    if (rc != DS2I_OK) return rc;
    IndexHandle idx(raw);
    DS2I_TRY
    const uint64_t V = idx->size, num_docs = idx->num_docs;
    std::vector<uint64_t> offs(V + 1);
    range_offsets(idx.get(), 0, V, offs.data());
    DevPostings dp;
    double ms_extract = 0.0, ms_encode = 0.0;
    rc = ds2i_extract_to_device(idx.get(), 0, V, offs.data(), dp, ms_extract);
    if (no_room) *no_room = rc == DS2I_ENOMEM;
    if (rc != DS2I_OK) return rc;
    idx.reset(); // the source image leaves the device before the sort's second buffers or the encoder's tables and output arrive
    double ms_remap[4] = {0.0, 0.0, 0.0, 0.0};
    if (doc_map) { // the documents renumbered where the postings lie (capi_remap.cpp); its temporaries are gone when it returns
        rc = ds2i_remap_device_postings(who, device, num_docs, V, offs.data(), dp, doc_map, ms_remap);
        if (rc != DS2I_OK) return rc;
    }
    uint32_t *d_docs = dp.docs, *d_freqs = dp.freqs;
    dp.release(); // (the encoder's staging owns them from here on)
    rc = ds2i_encode_device_postings(who, device, to_kind, num_docs, V, offs.data(), d_docs, d_freqs, out_image, &ms_encode);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = ms_extract + ms_remap[0] + ms_remap[1] + ms_remap[2] + ms_remap[3] + ms_encode;
    if (remap_ms) {
        std::copy(ms_remap, ms_remap + 4, remap_ms);
        remap_ms[4] = ms_extract;
        remap_ms[5] = ms_encode;
    }
    return DS2I_OK;
    DS2I_CATCH
}

extern "C" {

int ds2i_hip_index_extract(ds2i_hip_index* idx, uint64_t list_begin, uint64_t list_end, uint64_t* list_offsets, uint32_t* docs,
                           uint32_t* freqs, uint64_t capacity, uint64_t* postings, double* device_ms) {
    if (!idx || !list_offsets || !postings || (!docs) != (!freqs)) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_index_extract: null argument");
    if (list_begin > list_end || list_end > idx->size) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_index_extract: list range outside the index");
    if (device_ms) *device_ms = 0.0;
    range_offsets(idx, list_begin, list_end, list_offsets);
    const uint64_t total = list_offsets[list_end - list_begin];
    *postings = total;
    if (!docs) return DS2I_OK; // the size query
    if (capacity < total) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_index_extract: capacity too small");
    DevPostings dp;
    double ms = 0.0;
    const int rc = ds2i_extract_to_device(idx, list_begin, list_end, list_offsets, dp, ms);
    if (rc != DS2I_OK) return rc;
    HIP_OK(hipMemcpy(docs, dp.docs, 4 * total, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(freqs, dp.freqs, 4 * total, hipMemcpyDeviceToHost));
    if (device_ms) *device_ms = ms;
    return DS2I_OK;
}

int ds2i_hip_extract_collection(int device, int index_kind, const void* image, size_t bytes, uint64_t* num_docs, uint64_t* nlists,
                                ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs, double* device_ms) {
    if (!image || !num_docs || !nlists || !list_offsets || !docs || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_extract_collection: null argument");
    if (index_kind < DS2I_BLOCK_OPTPFOR || index_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_extract_collection: unknown index kind");
    extract_host_s[0] = extract_host_s[1] = extract_host_s[2] = 0.0;
    uint64_t img_docs = 0, img_lists = 0;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = ds2i_parse_image(index_kind, image, bytes, img_docs, img_lists, nullptr);
    if (rc != DS2I_OK) return rc;
    extract_host_s[0] = seconds_since(t0);
    rc = check_device("ds2i_hip_extract_collection", device);
    if (rc != DS2I_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    ds2i_hip_index* raw = nullptr;
    rc = ds2i_index_open_bare(device, index_kind, image, bytes, &raw);
    if (rc != DS2I_OK) return rc;
    IndexHandle idx(raw);
    extract_host_s[1] = seconds_since(t1);
    DS2I_TRY
    const uint64_t V = idx->size;
    std::unique_ptr<ds2i_blob> bo(new ds2i_blob), bd(new ds2i_blob), bf(new ds2i_blob);
    bo->data.resize(8 * (V + 1));
    uint64_t* offs = (uint64_t*)bo->data.data();
    range_offsets(idx.get(), 0, V, offs);
    const uint64_t total = offs[V];
    bd->data.resize(4 * total);
    bf->data.resize(4 * total);
    DevPostings dp;
    double ms = 0.0;
    rc = ds2i_extract_to_device(idx.get(), 0, V, offs, dp, ms);
    if (rc != DS2I_OK) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    HIP_OK(hipMemcpy(bd->data.data(), dp.docs, 4 * total, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bf->data.data(), dp.freqs, 4 * total, hipMemcpyDeviceToHost));
    extract_host_s[2] = seconds_since(t2);
    *num_docs = idx->num_docs;
    *nlists = V;
    *list_offsets = bo.release();
    *docs = bd.release();
    *freqs = bf.release();
    if (device_ms) *device_ms = ms;
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_convert_index(int device, int from_kind, const void* image, size_t bytes, int to_kind, ds2i_blob** out_image, double* device_ms) {
    if (!image || !out_image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_convert_index: null argument");
    if (from_kind < DS2I_BLOCK_OPTPFOR || from_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_convert_index: unknown index kind");
    int rc = ds2i_check_encoder_kind("ds2i_hip_convert_index", to_kind);
    if (rc != DS2I_OK) return rc;
    uint64_t num_docs = 0, nlists = 0;
    rc = ds2i_parse_image(from_kind, image, bytes, num_docs, nlists, nullptr);
    if (rc != DS2I_OK) return rc;
    rc = check_device("ds2i_hip_convert_index", device);
    if (rc != DS2I_OK) return rc;
    ds2i_blob* img = nullptr;
    rc = ds2i_convert_image("ds2i_hip_convert_index", device, from_kind, image, bytes, to_kind, &img, device_ms, nullptr);
    if (rc != DS2I_OK) return rc;
    *out_image = img;
    return DS2I_OK;
}

void ds2i_hip_extract_host_seconds(double seconds[3]) {
    if (seconds) std::memcpy(seconds, extract_host_s, sizeof extract_host_s);
}

} // extern "C"
