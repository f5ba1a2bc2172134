// Host side of ordering documents on the device (include/ds2i_hip.h: ds2i_hip_order_postings, ds2i_hip_order_index): the argument
// checks, all made on the host (host_order.hpp) before a device is looked for, and the level loop of recursive graph bisection over
// postings that lie on the device -- the launches of order_kernels.hip and, for the lists at a level's start and the halves in every
// iteration, the segmented sort of the remap (ds2i_remap_device_postings). The host reads one word an iteration, the exchanges; every
// level and iteration that the twin (host_order.hpp, order_postings) runs is run here, and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_util.hpp"
#include "host_order.hpp"
#include "launchers.hpp"

namespace {

using namespace ds2i_dev;
using ds2i_host::order_params;

// {extraction, level sort, runs, degrees, gains, gain sort, swap, compose}: hipEvent milliseconds of this thread's last ordering
// (ds2i_hip_order_ms)
thread_local double order_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};

double sum_ms() {
    double s = 0.0;
    for (double x : order_ms) s += x;
    return s;
}

// two fresh buffers of n words each (one unused word when n == 0: hipMalloc of 0 bytes gives no pointer to free)
bool alloc_pair(DevPostings& p, uint64_t n) {
    return hipMalloc((void**)&p.docs, 4 * std::max<uint64_t>(n, 1)) == hipSuccess && hipMalloc((void**)&p.freqs, 4 * std::max<uint64_t>(n, 1)) == hipSuccess;
}

// The level loop over checked postings on the device: dp.docs holds the doc-ids list by list (offs on the host), dp.freqs a word per
// posting whose content does not matter (it travels through the level sorts and holds `back` in between). At least level 0 runs.
int order_device(const char* who, int device, uint64_t n, uint64_t nlists, const uint64_t* offs, DevPostings& dp, order_params const& prm,
                 std::vector<uint32_t>& doc_map, std::vector<uint64_t>& trace) {
    const uint64_t total = offs[nlists];
    if (nlists >= (1ull << 32)) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": 2^32 lists or more").c_str());
    HIP_OK(hipSetDevice(device));
    int cus = 0;
    HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus <= 0) cus = 1;
    auto nomem = [&] {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": the ordering does not fit on the device (16 bytes per posting, 24 while the lists are sorted, "
                                                               "and 40 bytes per document, 48 while the halves are sorted)").c_str());
    };
    hipStream_t s = nullptr;
    DevTemps dev;
    DevPostings slots; // (keys, members): the pair the sort of the halves takes and may exchange for its second pair
    OrderArgs a{};
    uint32_t *d_logq = nullptr, *d_order = nullptr, *d_next = nullptr;
    uint64_t* d_first = nullptr;
    if (dev.alloc(&d_logq, 4 * (n + 3)) != hipSuccess || dev.alloc(&d_first, 8 * (nlists + 1)) != hipSuccess || dev.alloc(&a.run_len, 4 * total) != hipSuccess ||
        dev.alloc(&a.deg_right, 4 * total) != hipSuccess || dev.alloc(&a.half_of, 4 * n) != hipSuccess || dev.alloc(&a.side, 4 * n) != hipSuccess ||
        dev.alloc(&a.gain, 8 * n) != hipSuccess || dev.alloc(&d_order, 4 * n) != hipSuccess || dev.alloc(&d_next, 4 * n) != hipSuccess ||
        dev.alloc(&a.inv, 4 * n) != hipSuccess || dev.alloc(&a.exchanges, 8) != hipSuccess || dev.alloc(&a.flag, 4) != hipSuccess || !alloc_pair(slots, n))
        return nomem();
    {
        std::vector<uint32_t> logq(n + 3);
        ds2i_host::order_log_table(n + 3, logq.data());
        HIP_OK(hipMemcpy(d_logq, logq.data(), 4 * (n + 3), hipMemcpyHostToDevice));
        for (uint64_t x = 0; x < n; ++x) logq[x] = (uint32_t)x; // order starts as the identity
        HIP_OK(hipMemcpy(d_order, logq.data(), 4 * n, hipMemcpyHostToDevice));
    }
    HIP_OK(hipMemcpy(d_first, offs, 8 * (nlists + 1), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(a.flag, 0, 4));
    a.num_docs = n;
    a.logq = d_logq;
    a.postings = total;
    a.list_first = d_first;
    a.nlists = (uint32_t)nlists;
    const unsigned grid_entries = (unsigned)std::min<uint64_t>((total + SPLIT_THREADS - 1) / SPLIT_THREADS, 8ull * cus);
    const unsigned grid_windows = split_grid((total + ORDER_WINDOW - 1) / ORDER_WINDOW, cus);
    const unsigned grid_docs = (unsigned)std::min<uint64_t>((n + SPLIT_THREADS - 1) / SPLIT_THREADS, 8ull * cus);
    a.docs = dp.docs;
    HIP_OK(timed_span(s, order_ms[2], [&] { return ds2i_launch_order_check(a, grid_entries, s); }));
    uint32_t flag = 0;
    HIP_OK(hipMemcpy(&flag, a.flag, 4, hipMemcpyDeviceToHost));
    if (flag) return ds2i_set_error(DS2I_EFORMAT, (std::string(who) + ": a doc-id of the postings lies outside the " + std::to_string(n) + " documents").c_str());
    uint32_t bounds[3];
    ds2i_hip_remap_class_bounds(bounds);
    std::vector<uint64_t> half_first;
    double ms[4];
    for (uint32_t level = 0; ds2i_host::order_level_runs(n, level, prm); ++level) {
        a.level = level;
        a.order = d_order;
        a.next_order = d_next;
        if (level) { // the entries named by this level's p0, every list in order again
            HIP_OK(timed_span(s, order_ms[1], [&] { return ds2i_launch_order_renumber(a, grid_entries, s); }));
            const int rc = ds2i_remap_device_postings(who, device, n, nlists, offs, dp, nullptr, ms);
            order_ms[1] += ms[1] + ms[2] + ms[3];
            if (rc != DS2I_OK) return rc;
            a.docs = dp.docs; // (the sort may have exchanged the pair)
        }
        a.back = dp.freqs;
        a.keys = slots.docs;
        a.members = slots.freqs;
        HIP_OK(timed_span(s, order_ms[2], [&] {
            const hipError_t e = ds2i_launch_order_level(a, grid_docs, s);
            return e != hipSuccess ? e : ds2i_launch_order_runs(a, grid_windows, s);
        }));
        const uint64_t halves = 2ull << level;
        half_first.resize(halves + 1);
        uint64_t longest = 0;
        for (uint64_t h = 0; h <= halves; ++h) half_first[h] = ds2i_host::order_bound(n, level + 1, h);
        for (uint64_t h = 0; h < halves; ++h) longest = std::max(longest, half_first[h + 1] - half_first[h]);
        const bool presort = longest > bounds[1]; // a half in class 3: its sort by gain is only stable
        for (uint32_t it = 0; it < prm.iterations; ++it) {
            HIP_OK(timed_span(s, order_ms[3], [&] {
                const hipError_t e = hipMemsetAsync(a.deg_right, 0, 4 * std::max<uint64_t>(total, 1), s);
                return e != hipSuccess ? e : ds2i_launch_order_degrees(a, grid_windows, s);
            }));
            HIP_OK(timed_span(s, order_ms[4], [&] {
                const hipError_t e = hipMemsetAsync(a.gain, 0, 8 * std::max<uint64_t>(n, 1), s);
                return e != hipSuccess ? e : ds2i_launch_order_gains(a, grid_entries, s);
            }));
            if (presort) {
                HIP_OK(timed_span(s, order_ms[5], [&] { return ds2i_launch_order_presort_keys(a, grid_docs, s); }));
                const int rc = ds2i_remap_device_postings(who, device, n, halves, half_first.data(), slots, nullptr, ms);
                order_ms[5] += ms[1] + ms[2] + ms[3];
                if (rc != DS2I_OK) return rc;
                a.keys = slots.docs;
                a.members = slots.freqs;
            }
            HIP_OK(timed_span(s, order_ms[5], [&] { return ds2i_launch_order_keys(a, grid_docs, s); }));
            // the key bound is all 32 bits: a gain's image may be any word. The padding pair of the sort's networks is all ones, and
            // no (key, p0) pair equals it: p0 < n < 2^32 - 2.
            const int rc = ds2i_remap_device_postings(who, device, 0xFFFFFFFFull, halves, half_first.data(), slots, nullptr, ms);
            order_ms[5] += ms[1] + ms[2] + ms[3];
            if (rc != DS2I_OK) return rc;
            a.keys = slots.docs;
            a.members = slots.freqs;
            HIP_OK(timed_span(s, order_ms[6], [&] {
                const hipError_t e = hipMemsetAsync(a.exchanges, 0, 8, s);
                return e != hipSuccess ? e : ds2i_launch_order_swap(a, grid_docs, s);
            }));
            unsigned long long exchanges = 0;
            HIP_OK(hipMemcpy(&exchanges, a.exchanges, 8, hipMemcpyDeviceToHost));
            trace.push_back(exchanges);
            if (!exchanges) break;
        }
        HIP_OK(timed_span(s, order_ms[7], [&] { return ds2i_launch_order_compose(a, grid_docs, s); }));
        std::swap(d_order, d_next);
    }
    a.order = d_order;
    a.doc_map = d_next;
    HIP_OK(timed_span(s, order_ms[7], [&] { return ds2i_launch_order_finish(a, grid_docs, s); }));
    doc_map.resize(n);
    HIP_OK(hipMemcpy(doc_map.data(), a.doc_map, 4 * n, hipMemcpyDeviceToHost));
    return DS2I_OK;
}

void identity(uint64_t n, std::vector<uint32_t>& doc_map) {
    doc_map.resize(n);
    for (uint64_t d = 0; d < n; ++d) doc_map[d] = (uint32_t)d;
}

int params_fault(const char* who, uint64_t num_docs, const ds2i_order_params* p, order_params& prm) {
    std::string fault = ds2i_host::order_num_docs_fault(who, num_docs);
    if (fault.empty()) fault = ds2i_host::order_params_fault(who, p ? p->iterations : 0, p ? p->min_half : 0, p ? p->max_levels : 0, prm);
    return fault.empty() ? DS2I_OK : ds2i_set_error(DS2I_EINVAL, fault.c_str());
}

} // namespace

extern "C" {

int ds2i_hip_order_postings(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                            const ds2i_order_params* params, ds2i_blob** doc_map, ds2i_blob** trace, double* device_ms) {
    static const char* const who = "ds2i_hip_order_postings";
    if (!list_offsets || !docs || !doc_map || !trace) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_order_postings: null argument");
    DS2I_TRY
    std::string fault = ds2i_host::order_offsets_fault(who, nlists, list_offsets);
    if (!fault.empty()) return ds2i_set_error(DS2I_EINVAL, fault.c_str());
    fault = ds2i_host::order_docs_fault(who, num_docs, nlists, list_offsets, docs);
    if (!fault.empty()) return ds2i_set_error(DS2I_EFORMAT, fault.c_str());
    order_params prm;
    int rc = params_fault(who, num_docs, params, prm);
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(order_ms, order_ms + 8, 0.0);
    std::vector<uint32_t> map;
    std::vector<uint64_t> tr;
    if (!ds2i_host::order_level_runs(num_docs, 0, prm)) identity(num_docs, map);
    else {
        HIP_OK(hipSetDevice(device));
        const uint64_t total = list_offsets[nlists];
        DevPostings dp;
        if (!alloc_pair(dp, total)) {
            (void)hipGetLastError();
            return ds2i_set_error(DS2I_ENOMEM, "ds2i_hip_order_postings: the postings do not fit on the device (8 bytes per posting)");
        }
        if (total) HIP_OK(hipMemcpy(dp.docs, docs, 4 * total, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dp.freqs, 0, 4 * std::max<uint64_t>(total, 1)));
        rc = order_device(who, device, num_docs, nlists, list_offsets, dp, prm, map, tr);
        if (rc != DS2I_OK) return rc;
    }
    std::unique_ptr<ds2i_blob> bm(ds2i_blob_of(map)), bt(ds2i_blob_of(tr));
    *doc_map = bm.release();
    *trace = bt.release();
    if (device_ms) *device_ms = sum_ms(); // (like every output, written only when the call succeeds)
    return DS2I_OK;
    DS2I_CATCH
}

int ds2i_hip_order_index(int device, int index_kind, const void* image, size_t bytes, const ds2i_order_params* params, ds2i_blob** doc_map,
                         ds2i_blob** trace, double* device_ms) {
    static const char* const who = "ds2i_hip_order_index";
    if (!image || !doc_map || !trace) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_order_index: null argument");
    if (index_kind < DS2I_BLOCK_OPTPFOR || index_kind > DS2I_UNIFORM) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_order_index: unknown index kind");
    DS2I_TRY
    uint64_t num_docs = 0, nlists = 0;
    std::vector<uint32_t> lengths;
    int rc = ds2i_parse_image(index_kind, image, bytes, num_docs, nlists, &lengths);
    if (rc != DS2I_OK) return rc;
    order_params prm;
    rc = params_fault(who, num_docs, params, prm);
    if (rc != DS2I_OK) return rc;
    rc = check_device(who, device);
    if (rc != DS2I_OK) return rc;
    std::fill(order_ms, order_ms + 8, 0.0);
    std::vector<uint32_t> map;
    std::vector<uint64_t> tr;
    if (!ds2i_host::order_level_runs(num_docs, 0, prm)) identity(num_docs, map);
    else {
        std::vector<uint64_t> offs(nlists + 1, 0);
        for (uint64_t t = 0; t < nlists; ++t) offs[t + 1] = offs[t] + lengths[t];
        std::vector<uint32_t>().swap(lengths);
        DevPostings dp;
        {
            ds2i_hip_index* raw = nullptr;
            rc = ds2i_index_open_bare(device, index_kind, image, bytes, &raw);
            if (rc != DS2I_OK) return rc;
            IndexHandle idx(raw);
            rc = ds2i_extract_to_device(idx.get(), 0, nlists, offs.data(), dp, order_ms[0]);
            if (rc != DS2I_OK) return rc;
        } // (the image leaves the device before the ordering's tables arrive)
        rc = order_device(who, device, num_docs, nlists, offs.data(), dp, prm, map, tr);
        if (rc != DS2I_OK) return rc;
    }
    std::unique_ptr<ds2i_blob> bm(ds2i_blob_of(map)), bt(ds2i_blob_of(tr));
    *doc_map = bm.release();
    *trace = bt.release();
    if (device_ms) *device_ms = sum_ms(); // (like every output, written only when the call succeeds)
    return DS2I_OK;
    DS2I_CATCH
}

void ds2i_hip_order_ms(double ms[8]) {
    if (ms) std::memcpy(ms, order_ms, sizeof order_ms);
}

} // extern "C"
