// Host side of the extraction (include/ds2i_hip.h: ds2i_hip_index_extract, ds2i_hip_extract_collection, ds2i_hip_convert_index): the
// argument checks, the host parse of an image before any device is touched, ONE launch of k_extract_index[_side]
// (kernels_upload.inc: the verifier's whole-index walk with stores instead of compares) over the blocks of a range of lists, and
// what is done with the postings: copied to the caller, or handed to the index encoder where they lie (capi_encode.cpp,
// ds2i_encode_device_postings), so that a conversion between kinds never sends them over the bus.
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

using ds2i_dev::QTerm;

namespace {

// seconds of {image parse, bare upload of the image, copy of the postings to the host} of this thread's last
// ds2i_hip_extract_collection (ds2i_hip_extract_host_seconds)
thread_local double extract_host_s[3] = {0.0, 0.0, 0.0};
double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// the postings of a range of lists on the device: hipMalloc-ed, freed here unless released to another owner
struct DevPostings {
    uint32_t *docs = nullptr, *freqs = nullptr;
    DevPostings() {}
    DevPostings(DevPostings const&) = delete;
    DevPostings& operator=(DevPostings const&) = delete;
    ~DevPostings() {
        if (docs) (void)hipFree(docs);
        if (freqs) (void)hipFree(freqs);
    }
    void release() { docs = freqs = nullptr; }
};

// offs[0 .. end - begin] = where every list of [begin, end) starts in the output, from 0
void range_offsets(const ds2i_hip_index* idx, uint64_t begin, uint64_t end, uint64_t* offs) {
    offs[0] = 0;
    for (uint64_t t = begin; t < end; ++t) offs[t - begin + 1] = offs[t - begin] + idx->list_n[t];
}

// The postings of lists [begin, end) into two fresh device buffers of exactly offs[end - begin] postings each: one launch.
// ms accumulates the kernel's hipEvent time.
int extract_to_device(ds2i_hip_index* idx, uint64_t begin, uint64_t end, const uint64_t* offs, DevPostings& out, double& ms) {
    const uint64_t V = end - begin, total = offs[V];
    if (idx->total_blocks >= (1ull << 32)) return ds2i_set_error(DS2I_EINVAL, "index extraction: more than 2^32 blocks");
    HIP_OK(hipSetDevice(idx->device));
    // (hipMalloc of 0 bytes gives no pointer to free: the buffers of an empty range hold one unused word)
    if (hipMalloc((void**)&out.docs, 4 * std::max<uint64_t>(total, 1)) != hipSuccess || hipMalloc((void**)&out.freqs, 4 * std::max<uint64_t>(total, 1)) != hipSuccess) {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, "index extraction: the postings do not fit beside the index (8 bytes per posting)");
    }
    if (!V || !total) return DS2I_OK;
    const uint64_t block_begin = idx->list_blk_base[begin], block_end = idx->list_blk_base[end - 1] + idx->list_nb[end - 1];
    if (block_end <= block_begin) return DS2I_OK;
    std::vector<QTerm> lists;
    DS2I_TRY
    lists.resize(V);
    DS2I_CATCH
    for (uint64_t t = 0; t < V; ++t) lists[t] = ds2i_make_qterm(idx, (uint32_t)(begin + t));
    DevTemps dev;
    QTerm* d_lists = nullptr;
    uint64_t* d_first = nullptr;
    if (dev.alloc(&d_lists, sizeof(QTerm) * V) != hipSuccess || dev.alloc(&d_first, 8 * (V + 1)) != hipSuccess) {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, "index extraction: the postings do not fit beside the index (8 bytes per posting)");
    }
    HIP_OK(hipMemcpy(d_lists, lists.data(), sizeof(QTerm) * V, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_first, offs, 8 * (V + 1), hipMemcpyHostToDevice));
    ds2i_dev::ExtractArgs a{};
    a.arena = idx->d_arena;
    a.bits0 = idx->d_bits0;
    a.bits1 = idx->d_bits1;
    a.lists = d_lists;
    a.nlists = (uint32_t)V;
    a.block_begin = (uint32_t)block_begin;
    a.block_end = (uint32_t)block_end;
    a.codec = idx->kind >= DS2I_OPT ? (int)DS2I_OPT : idx->kind; // every freq_index layout decodes through the chunk directory
    a.num_docs = (uint32_t)idx->num_docs;
    a.out_docs = out.docs;
    a.out_freqs = out.freqs;
    a.list_first = d_first;
    a.skip = idx->d_skip;
    a.xslots = idx->d_xslots;
    a.xovf = idx->d_xovf;
    a.tails = idx->d_tails;
    const unsigned grid = (unsigned)std::min<uint64_t>(block_end - block_begin, uint64_t(idx->num_cus) * 16);
    // block_optpfor with side tables: through the stream kernels' decoder (DS2I_DECODE_GENERAL=1: the general decoders)
    const bool side = idx->side_tables() && !idx->knobs.decode_general;
    HIP_OK(timed_span(idx->stream[0], ms, [&] { return side ? ds2i_launch_extract_index_side(a, grid, idx->stream[0]) : ds2i_launch_extract_index(a, grid, idx->stream[0]); }));
    return DS2I_OK;
}

// The image on the host, as ds2i_hip_index_open reads it: number of documents, number of lists. A garbage image is DS2I_EFORMAT here,
// before a device is looked for.
int parse_image(int index_kind, const void* image, size_t bytes, uint64_t& num_docs, uint64_t& nlists) {
    DS2I_TRY
    if (ds2i_host::is_freq_layout(index_kind)) {
        ds2i_host::opt_index_view v;
        v.layout = index_kind;
        v.parse(image, bytes);
        num_docs = v.num_docs;
        nlists = v.size;
    } else {
        ds2i_host::block_index_view v;
        v.parse(image, bytes);
        num_docs = v.num_docs;
        nlists = v.size;
        for (uint64_t t = 0; t < v.size; ++t) {
            uint32_t n = 0;
            if (!ds2i_host_vbyte(v.lists + v.list_offsets[t], v.list_offsets[t + 1] - v.list_offsets[t], n) || !n)
                return ds2i_set_error(DS2I_EFORMAT, "posting list header is corrupt");
        }
    }
    return DS2I_OK;
    DS2I_CATCH
}

struct IndexCloser {
    void operator()(ds2i_hip_index* x) const { ds2i_hip_index_close(x); }
};
using IndexHandle = std::unique_ptr<ds2i_hip_index, IndexCloser>;

// null / kind checks, host parse, device check, bare upload: the common head of the two image entry points
int open_image_bare(const char* who, int device, int index_kind, const void* image, size_t bytes, IndexHandle& idx) {
    uint64_t num_docs = 0, nlists = 0;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = parse_image(index_kind, image, bytes, num_docs, nlists);
    if (rc != DS2I_OK) return rc;
    extract_host_s[0] = seconds_since(t0);
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    ds2i_hip_index* raw = nullptr;
    rc = ds2i_index_open_bare(device, index_kind, image, bytes, &raw);
    if (rc != DS2I_OK) return rc;
    idx.reset(raw);
    extract_host_s[1] = seconds_since(t1);
    return DS2I_OK;
}

} // namespace

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
    const int rc = extract_to_device(idx, list_begin, list_end, list_offsets, dp, ms);
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
    IndexHandle idx;
    int rc = open_image_bare("ds2i_hip_extract_collection", device, index_kind, image, bytes, idx);
    if (rc != DS2I_OK) return rc;
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
    rc = extract_to_device(idx.get(), 0, V, offs, dp, ms);
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
    IndexHandle idx;
    rc = open_image_bare("ds2i_hip_convert_index", device, from_kind, image, bytes, idx);
    if (rc != DS2I_OK) return rc;
    DS2I_TRY
    const uint64_t V = idx->size, num_docs = idx->num_docs;
    std::vector<uint64_t> offs(V + 1);
    range_offsets(idx.get(), 0, V, offs.data());
    DevPostings dp;
    double ms_extract = 0.0, ms_encode = 0.0;
    rc = extract_to_device(idx.get(), 0, V, offs.data(), dp, ms_extract);
    if (rc != DS2I_OK) return rc;
    idx.reset(); // the source image leaves the device before the encoder's tables and output arrive
    uint32_t *d_docs = dp.docs, *d_freqs = dp.freqs;
    dp.release(); // (the encoder's staging owns them from here on)
    ds2i_blob* img = nullptr;
    rc = ds2i_encode_device_postings("ds2i_hip_convert_index", device, to_kind, num_docs, V, offs.data(), d_docs, d_freqs, &img, &ms_encode);
    if (rc != DS2I_OK) return rc;
    *out_image = img;
    if (device_ms) *device_ms = ms_extract + ms_encode;
    return DS2I_OK;
    DS2I_CATCH
}

void ds2i_hip_extract_host_seconds(double seconds[3]) {
    if (seconds) std::memcpy(seconds, extract_host_s, sizeof extract_host_s);
}

} // extern "C"
