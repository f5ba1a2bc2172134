// Host side of renumbering documents on the device (include/ds2i_hip.h: ds2i_hip_remap_postings, ds2i_hip_remap_index): the argument
// checks, all made before a device is looked for, the plan of the segmented sort from the list lengths, and the launches of
// remap_kernels.hip over postings that lie on the device -- the map kernel, class 1, class 2, and class 3's radix passes, all on one
// stream. ds2i_remap_device_postings is the step ds2i_convert_image (capi_extract.cpp) takes between the extraction and the encoder
// when it is given a map, so that a remap is a conversion with one more step and the postings never cross the bus.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_util.hpp"
#include "launchers.hpp"

namespace {

using namespace ds2i_dev;

// {map, class 1, class 2, class 3, extraction, encoder}: hipEvent milliseconds of this thread's last remap (ds2i_hip_remap_ms)
thread_local double remap_ms[6] = {0, 0, 0, 0, 0, 0};

// The sort as the kernels take it (abi_structs.hpp, RemapArgs), from the list lengths alone: which lists a wavefront sorts, which a
// workgroup, and the tiles of the rest. A tile never spans two lists; a list's last tile is ragged.
struct SortPlan {
    std::vector<uint32_t> lists1, lists2;
    std::vector<RemapTile> tiles;
    std::vector<RemapLong> longs;
};

int plan_sort(const char* who, uint64_t nlists, const uint64_t* offs, SortPlan& p) {
    for (uint64_t t = 0; t < nlists; ++t) {
        const uint64_t first = offs[t], n = offs[t + 1] - first;
        if (!n) continue;
        if (n <= REMAP_W) p.lists1.push_back((uint32_t)t);
        else if (n <= REMAP_L) p.lists2.push_back((uint32_t)t);
        else {
            if (n > 0xFFFFFFFFull) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": a list of 2^32 postings or more").c_str());
            const uint64_t ntiles = (n + REMAP_T - 1) / REMAP_T;
            if (p.tiles.size() + ntiles > 0x7FFFFFFFull) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": more than 2^31 sort tiles").c_str());
            RemapLong l;
            l.first = first;
            l.tile0 = (uint32_t)p.tiles.size();
            l.ntiles = (uint32_t)ntiles;
            for (uint64_t k = 0; k < ntiles; ++k) {
                RemapTile tile;
                tile.first = first + k * REMAP_T;
                tile.count = (uint32_t)std::min<uint64_t>(REMAP_T, n - k * REMAP_T);
                tile.list3 = (uint32_t)p.longs.size();
                p.tiles.push_back(tile);
            }
            p.longs.push_back(l);
        }
    }
    return DS2I_OK;
}

template <class T>
int upload(DevTemps& dev, const T** out, std::vector<T> const& v) {
    T* d = nullptr;
    if (dev.alloc(&d, sizeof(T) * v.size()) != hipSuccess) return DS2I_ENOMEM;
    if (!v.empty()) HIP_OK(hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    *out = d;
    return DS2I_OK;
}

// the checks of a map that need no device: its length against the collection's, then that it is a permutation
int check_map(const char* who, const uint32_t* doc_map, uint64_t map_len, uint64_t num_docs) {
    if (map_len != num_docs)
        return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": the map holds " + std::to_string(map_len) + " documents, the collection " +
                                            std::to_string(num_docs)).c_str());
    return ds2i_check_doc_map(doc_map, num_docs);
}

} // namespace

int ds2i_remap_device_postings(const char* who, int device, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, DevPostings& dp,
                               const uint32_t* doc_map, double ms[4]) {
    ms[0] = ms[1] = ms[2] = ms[3] = 0.0;
    if (nlists >= (1ull << 32) || num_docs >= (1ull << 32)) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": 2^32 lists or documents, or more").c_str());
    const uint64_t total = offs[nlists];
    if (!total) return DS2I_OK;
    SortPlan plan;
    DS2I_TRY
    const int rc = plan_sort(who, nlists, offs, plan);
    if (rc != DS2I_OK) return rc;
    DS2I_CATCH
    HIP_OK(hipSetDevice(device));
    int cus = 0;
    HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus <= 0) cus = 1;
    auto nomem = [&] {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": the sort does not fit on the device (16 bytes per posting and 4 per document)").c_str());
    };
    DevTemps dev; // everything but the postings; the second buffer pair lives in `second` (one of the two pairs survives)
    DevPostings second;
    RemapArgs a{};
    uint32_t* d_map = nullptr;
    uint64_t* d_first = nullptr;
    if ((doc_map && dev.alloc(&d_map, 4 * num_docs) != hipSuccess) || dev.alloc(&d_first, 8 * (nlists + 1)) != hipSuccess || dev.alloc(&a.flag, 4) != hipSuccess)
        return nomem();
    int rc = upload(dev, &a.lists1, plan.lists1);
    if (rc == DS2I_OK) rc = upload(dev, &a.lists2, plan.lists2);
    if (rc == DS2I_OK) rc = upload(dev, &a.tiles, plan.tiles);
    if (rc == DS2I_OK) rc = upload(dev, &a.longs, plan.longs);
    if (rc == DS2I_ENOMEM) return nomem();
    if (rc != DS2I_OK) return rc;
    const bool radix = !plan.tiles.empty();
    if (radix && (hipMalloc((void**)&second.docs, 4 * total) != hipSuccess || hipMalloc((void**)&second.freqs, 4 * total) != hipSuccess ||
                  dev.alloc(&a.hist, (4ull << REMAP_DIGIT) * plan.tiles.size()) != hipSuccess))
        return nomem();
    if (doc_map) HIP_OK(hipMemcpy(d_map, doc_map, 4 * num_docs, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_first, offs, 8 * (nlists + 1), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(a.flag, 0, 4));
    // class 3 sorts the key bits the largest doc-id needs, REMAP_DIGIT a pass; an odd number of passes ends in the second pair
    uint32_t bits = 1;
    while (bits < 32 && ((num_docs - 1) >> bits)) ++bits;
    const uint32_t passes = radix ? (bits + REMAP_DIGIT - 1) / REMAP_DIGIT : 0;
    const bool ends_in_second = passes & 1;
    a.doc_map = d_map;
    a.num_docs = num_docs;
    a.postings = total;
    a.docs = dp.docs;
    a.freqs = dp.freqs;
    a.docs_b = second.docs;
    a.freqs_b = second.freqs;
    a.out_docs = ends_in_second ? second.docs : dp.docs;
    a.out_freqs = ends_in_second ? second.freqs : dp.freqs;
    a.list_first = d_first;
    a.nlists1 = (uint32_t)plan.lists1.size();
    a.nlists2 = (uint32_t)plan.lists2.size();
    a.ntiles = (uint32_t)plan.tiles.size();
    a.nlongs = (uint32_t)plan.longs.size();
    hipStream_t s = nullptr;
    // grids: workgroups of 256 threads that stride -- the map over the postings at up to 8 a compute unit, class 1 at 2 a compute unit
    // (8 waves, a list each), class 2 at 2 a compute unit, class 3 a tile a workgroup at up to 8 a compute unit
    const uint64_t wide = 8ull * cus, narrow = 2ull * cus;
    const unsigned grid_map = (unsigned)std::min<uint64_t>((total + 255) / 256, wide);
    const unsigned grid1 = (unsigned)std::min<uint64_t>((a.nlists1 + 3) / 4, narrow);
    const unsigned grid2 = (unsigned)std::min<uint64_t>(a.nlists2, narrow);
    const unsigned grid3 = (unsigned)std::min<uint64_t>(a.ntiles, wide);
    if (doc_map) { // (no map: the postings hold their new doc-ids already, as a merge leaves them, and only the sort runs)
        HIP_OK(timed_span(s, ms[0], [&] { return ds2i_launch_remap_map(a, grid_map, s); }));
        uint32_t flag = 0;
        HIP_OK(hipMemcpy(&flag, a.flag, 4, hipMemcpyDeviceToHost));
        if (flag) return ds2i_set_error(DS2I_EFORMAT, (std::string(who) + ": a doc-id of the postings lies outside the map").c_str());
    }
    if (a.nlists1) HIP_OK(timed_span(s, ms[1], [&] { return ds2i_launch_remap_sort1(a, grid1, s); }));
    if (a.nlists2) HIP_OK(timed_span(s, ms[2], [&] { return ds2i_launch_remap_sort2(a, grid2, s); }));
    if (radix)
        HIP_OK(timed_span(s, ms[3], [&] {
            for (uint32_t pass = 0; pass < passes; ++pass) {
                const hipError_t e = ds2i_launch_remap_radix_pass(a, pass & 1, pass * REMAP_DIGIT, grid3, s);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        }));
    if (ends_in_second) { // the sorted lists lie in the second pair: it becomes the caller's, the first is freed with `second`
        std::swap(dp.docs, second.docs);
        std::swap(dp.freqs, second.freqs);
    }
    return DS2I_OK; // (`second` and `dev` free the other pair and the tables here, before the encoder stages anything)
}

extern "C" {

int ds2i_hip_remap_postings(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                            const uint32_t* doc_map, uint32_t* out_docs, uint32_t* out_freqs, double* device_ms) {
    static const char* const who = "ds2i_hip_remap_postings";
    if (!list_offsets || !docs || !freqs || !doc_map || !out_docs || !out_freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_remap_postings: null argument");
    if (list_offsets[0] != 0) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_remap_postings: list_offsets must start at 0");
    for (uint64_t t = 0; t < nlists; ++t)
        if (list_offsets[t + 1] < list_offsets[t]) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_remap_postings: list_offsets decrease");
    int rc = ds2i_check_doc_map(doc_map, num_docs);
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = 0.0;
    std::fill(remap_ms, remap_ms + 6, 0.0);
    const uint64_t total = list_offsets[nlists];
    if (!total) return DS2I_OK;
    DS2I_TRY
    HIP_OK(hipSetDevice(device));
    DevPostings dp;
    if (hipMalloc((void**)&dp.docs, 4 * total) != hipSuccess || hipMalloc((void**)&dp.freqs, 4 * total) != hipSuccess) {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, "ds2i_hip_remap_postings: the postings do not fit on the device (8 bytes per posting)");
    }
    HIP_OK(hipMemcpy(dp.docs, docs, 4 * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dp.freqs, freqs, 4 * total, hipMemcpyHostToDevice));
    rc = ds2i_remap_device_postings(who, device, num_docs, nlists, list_offsets, dp, doc_map, remap_ms);
    if (rc != DS2I_OK) return rc;
    HIP_OK(hipMemcpy(out_docs, dp.docs, 4 * total, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_freqs, dp.freqs, 4 * total, hipMemcpyDeviceToHost));
    if (device_ms) *device_ms = remap_ms[0] + remap_ms[1] + remap_ms[2] + remap_ms[3];
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_remap_index(int device, int from_kind, const void* image, size_t bytes, const uint32_t* doc_map, uint64_t map_len, int to_kind,
                         ds2i_blob** out_image, double* device_ms) {
    static const char* const who = "ds2i_hip_remap_index";
    if (!image || !doc_map || !out_image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_remap_index: null argument");
    if (from_kind < DS2I_BLOCK_OPTPFOR || from_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_remap_index: unknown index kind");
    int rc = ds2i_check_encoder_kind(who, to_kind);
    if (rc != DS2I_OK) return rc;
    uint64_t num_docs = 0, nlists = 0;
    rc = ds2i_parse_image(from_kind, image, bytes, num_docs, nlists, nullptr);
    if (rc != DS2I_OK) return rc;
    DS2I_TRY
    rc = check_map(who, doc_map, map_len, num_docs);
    DS2I_CATCH
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(remap_ms, remap_ms + 6, 0.0);
    ds2i_blob* img = nullptr;
    rc = ds2i_convert_image(who, device, from_kind, image, bytes, to_kind, &img, device_ms, nullptr, doc_map, remap_ms);
    if (rc != DS2I_OK) return rc;
    *out_image = img;
    return DS2I_OK;
}

void ds2i_hip_remap_ms(double ms[6]) {
    if (ms) std::memcpy(ms, remap_ms, sizeof remap_ms);
}

} // extern "C"
