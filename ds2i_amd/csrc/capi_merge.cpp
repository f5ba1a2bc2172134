// Host side of merging indexes on the device (include/ds2i_hip.h: ds2i_hip_merge_indexes, ds2i_hip_merge_postings): the argument checks,
// all made on the host parse and the plan (host_merge.hpp) before a device is looked for, and the steps over postings that lie on the
// device: every source in turn brought there (extracted from its image, or copied up), placed among the merged postings by
// k_merge_place (merge_kernels.hip) and freed; the merged lists sorted by the segmented sort of the remap (capi_remap.cpp,
// ds2i_remap_device_postings without a map) unless the concatenated doc maps are the identity; and the encoder where they lie.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_util.hpp"
#include "host_merge.hpp"
#include "launchers.hpp"

namespace {

using namespace ds2i_dev;
using ds2i_host::merge_plan;
using ds2i_host::merge_shape;

// {extraction, placement, sort classes 1..3 summed, encoder, padding}: hipEvent milliseconds of this thread's last merge (ds2i_hip_merge_ms)
thread_local double merge_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// the merged postings on the device and what every source's placement shares
struct Merged {
    const char* who;
    int device, cus = 1;
    DevPostings dp;
    DevTemps dev;
    uint32_t* d_flag = nullptr;
    Merged(const char* who_, int device_) : who(who_), device(device_) {}
    int nomem() const {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": the merged postings and one source do not fit on the device (8 bytes per posting)").c_str());
    }
    int open(merge_plan const& plan) {
        HIP_OK(hipSetDevice(device));
        HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        if (cus <= 0) cus = 1;
        const uint64_t total = plan.offs[plan.nlists];
        // (hipMalloc of 0 bytes gives no pointer to free: the buffers of an empty merge hold one unused word)
        if (hipMalloc((void**)&dp.docs, 4 * std::max<uint64_t>(total, 1)) != hipSuccess ||
            hipMalloc((void**)&dp.freqs, 4 * std::max<uint64_t>(total, 1)) != hipSuccess || dev.alloc(&d_flag, 4) != hipSuccess)
            return nomem();
        HIP_OK(hipMemset(d_flag, 0, 4));
        return DS2I_OK;
    }
    // source s, its postings in `src` on the device, stored at their places; the tables of the launch are freed before this returns
    int place(merge_plan const& plan, uint32_t s, merge_shape const& m, DevPostings const& src) {
        const uint64_t total = m.offs[m.nlists];
        if (!total) return DS2I_OK;
        DevTemps tmp;
        uint64_t *d_src_first = nullptr, *d_dst_first = nullptr;
        uint32_t* d_map = nullptr;
        if (tmp.alloc(&d_src_first, 8 * (m.nlists + 1)) != hipSuccess || tmp.alloc(&d_dst_first, 8 * m.nlists) != hipSuccess ||
            (m.doc_map && tmp.alloc(&d_map, 4 * m.num_docs) != hipSuccess))
            return nomem();
        HIP_OK(hipMemcpy(d_src_first, m.offs, 8 * (m.nlists + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_dst_first, plan.dst_first[s].data(), 8 * m.nlists, hipMemcpyHostToDevice));
        if (m.doc_map) HIP_OK(hipMemcpy(d_map, m.doc_map, 4 * m.num_docs, hipMemcpyHostToDevice));
        MergePlaceArgs a{};
        a.src_docs = src.docs;
        a.src_freqs = src.freqs;
        a.dst_docs = dp.docs;
        a.dst_freqs = dp.freqs;
        a.src_first = d_src_first;
        a.dst_first = d_dst_first;
        a.doc_map = d_map;
        a.map_len = m.num_docs;
        a.postings = total;
        a.base = (uint32_t)plan.base[s];
        a.nlists = (uint32_t)m.nlists;
        a.flag = d_flag;
        // workgroups of 256 threads, four wavefronts, a window each at a time: up to 8 a compute unit, which stride
        const uint64_t windows = (total + MERGE_WINDOW - 1) / MERGE_WINDOW;
        const unsigned grid = (unsigned)std::min<uint64_t>((windows + 3) / 4, 8ull * cus);
        hipStream_t stream = nullptr;
        HIP_OK(timed_span(stream, merge_ms[1], [&] { return ds2i_launch_merge_place(a, grid, stream); }));
        uint32_t flag = 0;
        HIP_OK(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
        if (flag)
            return ds2i_set_error(DS2I_EFORMAT, (std::string(who) + ": a doc-id of source " + std::to_string(s) + " lies outside the map").c_str());
        return DS2I_OK;
    }
    // every merged list in doc-id order: nothing to do when the concatenated maps are the identity
    int sort(merge_plan const& plan) {
        if (plan.identity) return DS2I_OK;
        double ms[4];
        const int rc = ds2i_remap_device_postings(who, device, plan.num_docs, plan.nlists, plan.offs.data(), dp, nullptr, ms);
        merge_ms[2] = ms[1] + ms[2] + ms[3];
        return rc;
    }
};

} // namespace

extern "C" {

int ds2i_hip_merge_postings(int device, const ds2i_merge_postings_source* src, uint32_t nsrc, uint64_t nlists, uint64_t* num_docs, uint64_t* out_nlists,
                            ds2i_blob** list_offsets, ds2i_blob** docs, ds2i_blob** freqs, double* device_ms) {
    static const char* const who = "ds2i_hip_merge_postings";
    if (!num_docs || !out_nlists || !list_offsets || !docs || !freqs) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_merge_postings: null argument");
    DS2I_TRY
    std::vector<merge_shape> shapes;
    merge_plan plan;
    std::string fault = ds2i_host::merge_csr_fault(who, src, nsrc, shapes);
    if (fault.empty()) fault = ds2i_host::merge_plan_fault(who, shapes.data(), nsrc, nlists, plan);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    int rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = 0.0;
    std::fill(merge_ms, merge_ms + 8, 0.0);
    const uint64_t total = plan.offs[plan.nlists];
    std::unique_ptr<ds2i_blob> bo(new ds2i_blob), bd(new ds2i_blob), bf(new ds2i_blob);
    bo->data.resize(8 * (plan.nlists + 1));
    std::memcpy(bo->data.data(), plan.offs.data(), 8 * (plan.nlists + 1));
    bd->data.resize(4 * total);
    bf->data.resize(4 * total);
    Merged m(who, device);
    rc = m.open(plan);
    if (rc != DS2I_OK) return rc;
    for (uint32_t s = 0; s < nsrc; ++s) {
        const uint64_t n = shapes[s].offs[shapes[s].nlists];
        if (!n) continue;
        DevPostings up; // this source alone: gone before the next one arrives
        if (hipMalloc((void**)&up.docs, 4 * n) != hipSuccess || hipMalloc((void**)&up.freqs, 4 * n) != hipSuccess) return m.nomem();
        HIP_OK(hipMemcpy(up.docs, src[s].docs, 4 * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(up.freqs, src[s].freqs, 4 * n, hipMemcpyHostToDevice));
        rc = m.place(plan, s, shapes[s], up);
        if (rc != DS2I_OK) return rc;
    }
    rc = m.sort(plan);
    if (rc != DS2I_OK) return rc;
    if (total) {
        HIP_OK(hipMemcpy(bd->data.data(), m.dp.docs, 4 * total, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(bf->data.data(), m.dp.freqs, 4 * total, hipMemcpyDeviceToHost));
    }
    *num_docs = plan.num_docs;
    *out_nlists = plan.nlists;
    *list_offsets = bo.release();
    *docs = bd.release();
    *freqs = bf.release();
    if (device_ms) *device_ms = merge_ms[1] + merge_ms[2];
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_merge_indexes(int device, const ds2i_merge_source* src, uint32_t nsrc, uint64_t nlists, int to_kind, ds2i_blob** out_image,
                           double* device_ms) {
    static const char* const who = "ds2i_hip_merge_indexes";
    if (!src || !out_image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_merge_indexes: null argument");
    for (uint32_t s = 0; s < nsrc; ++s)
        if (!src[s].image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_merge_indexes: null argument");
    if (!nsrc) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_merge_indexes: no source");
    for (uint32_t s = 0; s < nsrc; ++s)
        if (src[s].kind < DS2I_BLOCK_OPTPFOR || src[s].kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_merge_indexes: unknown index kind");
    int rc = ds2i_check_encoder_kind(who, to_kind);
    if (rc != DS2I_OK) return rc;
    DS2I_TRY
    std::vector<merge_shape> shapes(nsrc);
    std::vector<std::vector<uint64_t>> offs(nsrc);
    for (uint32_t s = 0; s < nsrc; ++s) {
        std::vector<uint32_t> lengths;
        merge_shape& m = shapes[s];
        rc = ds2i_parse_image(src[s].kind, src[s].image, src[s].bytes, m.num_docs, m.nlists, &lengths);
        if (rc != DS2I_OK) return rc;
        offs[s].assign(m.nlists + 1, 0);
        for (uint64_t t = 0; t < m.nlists; ++t) offs[s][t + 1] = offs[s][t] + lengths[t];
        m.offs = offs[s].data();
        m.doc_map = src[s].doc_map;
        m.map_len = src[s].map_len;
        m.term_map = src[s].term_map;
        m.terms_len = src[s].terms_len;
    }
    merge_plan plan;
    const std::string fault = ds2i_host::merge_plan_fault(who, shapes.data(), nsrc, nlists, plan);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    if (device_ms) *device_ms = 0.0;
    std::fill(merge_ms, merge_ms + 8, 0.0);
    Merged m(who, device);
    rc = m.open(plan);
    if (rc != DS2I_OK) return rc;
    for (uint32_t s = 0; s < nsrc; ++s) {
        ds2i_hip_index* raw = nullptr;
        rc = ds2i_index_open_bare(device, src[s].kind, src[s].image, src[s].bytes, &raw);
        if (rc != DS2I_OK) return rc;
        IndexHandle idx(raw);
        DevPostings from; // this source alone: gone before the next one arrives
        rc = ds2i_extract_to_device(idx.get(), 0, shapes[s].nlists, shapes[s].offs, from, merge_ms[0]);
        if (rc != DS2I_OK) return rc;
        idx.reset(); // the image leaves the device before the placement's tables arrive
        rc = m.place(plan, s, shapes[s], from);
        if (rc != DS2I_OK) return rc;
    }
    rc = m.sort(plan);
    if (rc != DS2I_OK) return rc;
    uint32_t *d_docs = m.dp.docs, *d_freqs = m.dp.freqs;
    m.dp.release(); // (the encoder's staging owns them from here on)
    ds2i_blob* img = nullptr;
    rc = ds2i_encode_device_postings(who, device, to_kind, plan.num_docs, plan.nlists, plan.offs.data(), d_docs, d_freqs, &img, &merge_ms[3]);
    if (rc != DS2I_OK) return rc;
    *out_image = img;
    if (device_ms) *device_ms = merge_ms[0] + merge_ms[1] + merge_ms[2] + merge_ms[3];
    return DS2I_OK;
    DS2I_CATCH
}

void ds2i_hip_merge_ms(double ms[4 + 4]) {
    if (ms) std::memcpy(ms, merge_ms, sizeof merge_ms);
}

} // extern "C"
