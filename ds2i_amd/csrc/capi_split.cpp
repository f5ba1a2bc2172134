// Host side of splitting an index on the device (include/ds2i_hip.h: ds2i_hip_split_index, ds2i_hip_split_postings), the inverse of
// capi_merge.cpp: the argument checks, all made on the host (host_split.hpp) before a device is looked for, and the steps over postings
// that lie on the device: the source brought there once (extracted from its image, or copied up) with shard_of and the table of local
// ids, then every shard in turn cut out of it by the three kernels of split_kernels.hip -- count, the scan of the window counts on the
// host, scatter into buffers of exactly the shard's size, offsets -- and encoded where it lies, or copied down.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_split.hpp"
#include "capi_util.hpp"
#include "host_split.hpp"
#include "launchers.hpp"

namespace {

using namespace ds2i_dev;
using ds2i_host::split_shard;

// {extraction, count, offsets, scatter, encoder, padding}: hipEvent milliseconds of this thread's last split (ds2i_hip_split_ms)
thread_local double split_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// what every shard of one split shares on the device -- shard_of, the local ids, the source's list starts, the window tables -- and
// the steps of one shard over the source postings `src`
struct Splitter {
    const char* who;
    int device, cus = 1;
    uint64_t num_docs, nlists, postings, windows;
    const uint64_t* offs;
    DevTemps dev;
    SplitArgs a{};
    uint32_t* d_win_count = nullptr;
    uint64_t *d_win_base = nullptr, *d_kept_before = nullptr;
    std::vector<uint32_t> win_count;
    std::vector<uint64_t> win_base, kept_before;
    Splitter(const char* who_, int device_, uint64_t num_docs_, uint64_t nlists_, const uint64_t* offs_)
        : who(who_), device(device_), num_docs(num_docs_), nlists(nlists_), postings(offs_[nlists_]),
          windows((offs_[nlists_] + SPLIT_WINDOW - 1) / SPLIT_WINDOW), offs(offs_) {}
    int nomem() const {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": the source postings, the tables of the split (8 bytes per document) and one shard's "
                                                               "postings do not fit on the device (8 bytes per posting)").c_str());
    }
    // the tables go up once, for all shards
    int open(const uint32_t* shard_of, std::vector<uint32_t> const& local, DevPostings const& src) {
        HIP_OK(hipSetDevice(device));
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        uint32_t *d_shard_of = nullptr, *d_local = nullptr, *d_flag = nullptr;
        uint64_t* d_src_first = nullptr;
        if (dev.alloc(&d_shard_of, 4 * num_docs) != hipSuccess || dev.alloc(&d_local, 4 * num_docs) != hipSuccess ||
            dev.alloc(&d_src_first, 8 * (nlists + 1)) != hipSuccess || dev.alloc(&d_kept_before, 8 * (nlists + 1)) != hipSuccess ||
            dev.alloc(&d_win_count, 4 * windows) != hipSuccess || dev.alloc(&d_win_base, 8 * (windows + 1)) != hipSuccess ||
            dev.alloc(&d_flag, 4) != hipSuccess)
            return nomem();
        if (num_docs) {
            HIP_OK(hipMemcpy(d_shard_of, shard_of, 4 * num_docs, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(d_local, local.data(), 4 * num_docs, hipMemcpyHostToDevice));
        }
        HIP_OK(hipMemcpy(d_src_first, offs, 8 * (nlists + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_flag, 0, 4));
        win_count.resize(windows);
        win_base.resize(windows + 1);
        kept_before.resize(nlists + 1);
        a.src_docs = src.docs;
        a.src_freqs = src.freqs;
        a.postings = postings;
        a.shard_of = d_shard_of;
        a.local = d_local;
        a.num_docs = num_docs;
        a.nstarts = nlists + 1;
        a.win_count = d_win_count;
        a.win_base = d_win_base;
        a.src_first = d_src_first;
        a.kept_before = d_kept_before;
        a.flag = d_flag;
        return DS2I_OK;
    }
    // shard s counted: win_base scanned on the host (u64: a collection holds more than 2^32 postings) and back on the device; `kept`
    // receives the shard's postings
    int count(uint32_t s, uint64_t& kept) {
        a.shard = s;
        hipStream_t stream = nullptr;
        HIP_OK(timed_span(stream, split_ms[1], [&] { return ds2i_launch_split_count(a, split_grid(windows, cus), stream); }));
        uint32_t flag = 0;
        HIP_OK(hipMemcpy(&flag, a.flag, 4, hipMemcpyDeviceToHost));
        if (flag)
            return ds2i_set_error(DS2I_EFORMAT, (std::string(who) + ": a doc-id among the postings lies outside the " + std::to_string(num_docs) +
                                                 " documents").c_str());
        if (windows) HIP_OK(hipMemcpy(win_count.data(), d_win_count, 4 * windows, hipMemcpyDeviceToHost));
        win_base[0] = 0;
        for (uint64_t w = 0; w < windows; ++w) win_base[w + 1] = win_base[w] + win_count[w];
        HIP_OK(hipMemcpy(d_win_base, win_base.data(), 8 * (windows + 1), hipMemcpyHostToDevice));
        kept = win_base[windows];
        return DS2I_OK;
    }
    // shard s, counted, cut out: its postings into fresh buffers of exactly `kept` postings, its lists and term map into `sh`
    int cut(uint64_t kept, DevPostings& out, split_shard& sh) {
        // (hipMalloc of 0 bytes gives no pointer to free: the buffers of an empty shard hold one unused word)
        if (hipMalloc((void**)&out.docs, 4 * std::max<uint64_t>(kept, 1)) != hipSuccess ||
            hipMalloc((void**)&out.freqs, 4 * std::max<uint64_t>(kept, 1)) != hipSuccess)
            return nomem();
        a.dst_docs = out.docs;
        a.dst_freqs = out.freqs;
        hipStream_t stream = nullptr;
        if (kept) HIP_OK(timed_span(stream, split_ms[3], [&] { return ds2i_launch_split_scatter(a, split_grid(windows, cus), stream); }));
        HIP_OK(timed_span(stream, split_ms[2], [&] { return ds2i_launch_split_offsets(a, split_grid(nlists + 1, cus), stream); }));
        HIP_OK(hipMemcpy(kept_before.data(), d_kept_before, 8 * (nlists + 1), hipMemcpyDeviceToHost));
        if (kept_before[0] != 0 || kept_before[nlists] != kept)
            return ds2i_set_error(DS2I_EDEVICE, (std::string(who) + ": the offsets kernel and the count kernel disagree").c_str());
        ds2i_host::split_shard_lists(nlists, kept_before.data(), sh);
        return DS2I_OK;
    }
};

// the twin's checks of a collection in CSR form, then nothing
int check_csr(const char* who, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* shard_of, uint32_t nshards) {
    std::string fault = ds2i_host::split_csr_fault(who, nlists, offs);
    if (fault.empty()) fault = ds2i_host::split_assign_fault(who, num_docs, nlists, shard_of, nshards);
    return fault.empty() ? DS2I_OK : ds2i_set_error(DS2I_EINVAL, fault.c_str());
}

} // namespace

extern "C" {

int ds2i_hip_split_postings(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                            const uint32_t* shard_of, uint32_t nshards, ds2i_split_shard** shards, double* device_ms) {
    static const char* const who = "ds2i_hip_split_postings";
    if (!list_offsets || !docs || !freqs || (!shard_of && num_docs) || !shards) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_split_postings: null argument");
    DS2I_TRY
    int rc = check_csr(who, num_docs, nlists, list_offsets, shard_of, nshards);
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = 0.0;
    std::fill(split_ms, split_ms + 8, 0.0);
    std::vector<uint32_t> local;
    std::vector<std::vector<uint32_t>> doc_maps;
    ds2i_host::split_tables(num_docs, shard_of, nshards, local, doc_maps);
    Splitter sp(who, device, num_docs, nlists, list_offsets);
    HIP_OK(hipSetDevice(device));
    DevPostings src;
    if (hipMalloc((void**)&src.docs, 4 * std::max<uint64_t>(sp.postings, 1)) != hipSuccess ||
        hipMalloc((void**)&src.freqs, 4 * std::max<uint64_t>(sp.postings, 1)) != hipSuccess)
        return sp.nomem();
    if (sp.postings) {
        HIP_OK(hipMemcpy(src.docs, docs, 4 * sp.postings, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(src.freqs, freqs, 4 * sp.postings, hipMemcpyHostToDevice));
    }
    rc = sp.open(shard_of, local, src);
    if (rc != DS2I_OK) return rc;
    SplitShards arr = new_split_shards(nshards);
    for (uint32_t s = 0; s < nshards; ++s) {
        uint64_t kept = 0;
        rc = sp.count(s, kept);
        if (rc != DS2I_OK) return rc;
        DevPostings cutout; // this shard alone: gone before the next one is cut
        split_shard sh;
        rc = sp.cut(kept, cutout, sh);
        if (rc != DS2I_OK) return rc;
        sh.docs.resize(kept);
        sh.freqs.resize(kept);
        if (kept) {
            HIP_OK(hipMemcpy(sh.docs.data(), cutout.docs, 4 * kept, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(sh.freqs.data(), cutout.freqs, 4 * kept, hipMemcpyDeviceToHost));
        }
        sh.num_docs = doc_maps[s].size();
        sh.doc_map.swap(doc_maps[s]);
        fill_split_shard(arr.get()[s], sh, true);
    }
    *shards = arr.release();
    if (device_ms) *device_ms = split_ms[1] + split_ms[2] + split_ms[3];
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_split_index(int device, int from_kind, const void* image, size_t bytes, const uint32_t* shard_of, uint64_t map_len, uint32_t nshards,
                         int to_kind, ds2i_split_shard** shards, double* device_ms) {
    static const char* const who = "ds2i_hip_split_index";
    if (!image || !shard_of || !shards) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_split_index: null argument");
    if (!nshards) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_split_index: no shard");
    if (from_kind < DS2I_BLOCK_OPTPFOR || from_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_split_index: unknown index kind");
    int rc = ds2i_check_encoder_kind(who, to_kind);
    if (rc != DS2I_OK) return rc;
    DS2I_TRY
    uint64_t num_docs = 0, nlists = 0;
    std::vector<uint32_t> lengths;
    rc = ds2i_parse_image(from_kind, image, bytes, num_docs, nlists, &lengths);
    if (rc != DS2I_OK) return rc;
    if (map_len != num_docs)
        return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": shard_of holds " + std::to_string(map_len) + " documents, the index " +
                                            std::to_string(num_docs)).c_str());
    const std::string fault = ds2i_host::split_assign_fault(who, num_docs, nlists, shard_of, nshards);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    std::vector<uint32_t> local;
    std::vector<std::vector<uint32_t>> doc_maps;
    ds2i_host::split_tables(num_docs, shard_of, nshards, local, doc_maps);
    for (uint32_t s = 0; s < nshards; ++s)
        if (doc_maps[s].empty()) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": shard " + std::to_string(s) + " is assigned no document").c_str());
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = 0.0;
    std::fill(split_ms, split_ms + 8, 0.0);
    std::vector<uint64_t> offs(nlists + 1, 0);
    for (uint64_t t = 0; t < nlists; ++t) offs[t + 1] = offs[t] + lengths[t];
    std::vector<uint32_t>().swap(lengths);
    DevPostings src; // freed after the last shard
    {
        ds2i_hip_index* raw = nullptr;
        rc = ds2i_index_open_bare(device, from_kind, image, bytes, &raw);
        if (rc != DS2I_OK) return rc;
        IndexHandle idx(raw);
        rc = ds2i_extract_to_device(idx.get(), 0, nlists, offs.data(), src, split_ms[0]);
        if (rc != DS2I_OK) return rc;
    } // (the image leaves the device before the tables of the split arrive)
    Splitter sp(who, device, num_docs, nlists, offs.data());
    rc = sp.open(shard_of, local, src);
    if (rc != DS2I_OK) return rc;
    SplitShards arr = new_split_shards(nshards);
    for (uint32_t s = 0; s < nshards; ++s) {
        uint64_t kept = 0;
        rc = sp.count(s, kept);
        if (rc != DS2I_OK) return rc;
        if (!kept)
            return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": shard " + std::to_string(s) + " receives no posting: List must be nonempty").c_str());
        DevPostings cutout;
        split_shard sh;
        rc = sp.cut(kept, cutout, sh);
        if (rc != DS2I_OK) return rc;
        uint32_t *d_docs = cutout.docs, *d_freqs = cutout.freqs;
        cutout.release(); // (the encoder's staging owns them from here on)
        ds2i_blob* img = nullptr;
        double encoder_ms = 0.0;
        rc = ds2i_encode_device_postings(who, device, to_kind, doc_maps[s].size(), sh.nlists, sh.offs.data(), d_docs, d_freqs, &img, &encoder_ms);
        if (rc != DS2I_OK) return rc;
        split_ms[4] += encoder_ms;
        arr.get()[s].image = img;
        sh.num_docs = doc_maps[s].size();
        sh.doc_map.swap(doc_maps[s]);
        fill_split_shard(arr.get()[s], sh, false);
    }
    *shards = arr.release();
    if (device_ms) *device_ms = split_ms[0] + split_ms[1] + split_ms[2] + split_ms[3] + split_ms[4];
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_image_shape(int index_kind, const void* image, size_t bytes, uint64_t* num_docs, uint64_t* nlists) {
    if (!image || !num_docs || !nlists) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_image_shape: null argument");
    if (index_kind < DS2I_BLOCK_OPTPFOR || index_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_image_shape: unknown index kind");
    uint64_t docs = 0, lists = 0;
    const int rc = ds2i_parse_image(index_kind, image, bytes, docs, lists, nullptr);
    if (rc != DS2I_OK) return rc;
    *num_docs = docs;
    *nlists = lists;
    return DS2I_OK;
}

void ds2i_hip_split_ms(double ms[8]) {
    if (ms) std::memcpy(ms, split_ms, sizeof split_ms);
}

} // extern "C"
