// What the build-side C-ABI units share (capi.cpp: upload; capi_encode.cpp: encoders, wand data, optimiser; capi_verify.cpp;
// capi_extract.cpp): device temporaries, the timed span around a launch, the device check, the host's half of the whole-index walk,
// and the steps from an image to its postings on the device that the conversion and the transcoding upload share. (The exception guard is capi_error.hpp's DS2I_TRY / DS2I_CATCH,
// which the HIP-free capi_build.cpp uses too.)
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "capi_internal.hpp"

// device temporaries of one function (or one staging): freed on every path out of it
struct DevTemps {
    std::vector<void*> p;
    DevTemps() {}
    DevTemps(DevTemps const&) = delete;
    DevTemps& operator=(DevTemps const&) = delete;
    ~DevTemps() { for (void* x : p) if (x) (void)hipFree(x); }
    template <class T> hipError_t alloc(T** out, size_t bytes) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) p.push_back(q);
        *out = (T*)q;
        return e;
    }
};

// ms += the hipEvent time of what `launch()` (-> hipError_t) puts on `stream`: record, launch, record, synchronise. Returns the first
// HIP error; the two events are destroyed on every path.
template <class Launch>
hipError_t timed_span(hipStream_t stream, double& ms, Launch&& launch) {
    struct Events {
        hipEvent_t e[2] = {};
        ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    hipError_t rc;
    if ((rc = hipEventCreate(&ev.e[0])) != hipSuccess || (rc = hipEventCreate(&ev.e[1])) != hipSuccess) return rc;
    if ((rc = hipEventRecord(ev.e[0], stream)) != hipSuccess) return rc;
    if ((rc = launch()) != hipSuccess) return rc;
    if ((rc = hipEventRecord(ev.e[1], stream)) != hipSuccess || (rc = hipEventSynchronize(ev.e[1])) != hipSuccess) return rc;
    float t = 0.f;
    if ((rc = hipEventElapsedTime(&t, ev.e[0], ev.e[1])) != hipSuccess) return rc;
    ms += t;
    return hipSuccess;
}

// DS2I_OK, or DS2I_EDEVICE "<who>: no such HIP device"
inline int check_device(const char* who, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return ds2i_set_error(DS2I_EDEVICE, (std::string(who) + ": no such HIP device").c_str());
    return DS2I_OK;
}

// a handle that ds2i_hip_index_close releases on every path out (the bare uploads of the image entry points)
struct IndexCloser {
    void operator()(ds2i_hip_index* x) const { ds2i_hip_index_close(x); }
};
using IndexHandle = std::unique_ptr<ds2i_hip_index, IndexCloser>;

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

// The host's half of the whole-index walk (abi_structs.hpp, WalkArgs; kernels_upload.inc, walk_index[_side]), stated once for the
// verification and the extraction: the lists [begin, end) as the kernels see them and their posting offsets go up, the index's
// view and the block range are filled in, and the launch takes the side tables' kernel or the general one, a wave per block,
// inside a timed span. `who` ("index verification") and `misfit` ("the collection does not fit") make the error texts.
struct WalkStaging {
    const char *who, *misfit;
    DevTemps dev; // the staged lists and offsets; what else the caller stages for the walk may live here too
    ds2i_dev::WalkArgs w{};
    WalkStaging(const char* who_, const char* misfit_) : who(who_), misfit(misfit_) {}
    int nomem() const {
        (void)hipGetLastError();
        return ds2i_set_error(DS2I_ENOMEM, (std::string(who) + ": " + misfit + " beside the index (8 bytes per posting)").c_str());
    }
    uint64_t blocks() const { return w.block_end - w.block_begin; }
    // offs[0 .. end - begin]: where every list of the range starts among the postings, from 0. An empty range stages nothing.
    int stage(const ds2i_hip_index* idx, uint64_t begin, uint64_t end, const uint64_t* offs) {
        if (idx->total_blocks >= (1ull << 32)) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": more than 2^32 blocks").c_str());
        HIP_OK(hipSetDevice(idx->device));
        const uint64_t V = end - begin;
        w.v = ds2i_index_view(idx);
        if (!V) return DS2I_OK;
        w.nlists = (uint32_t)V;
        w.block_begin = (uint32_t)idx->list_blk_base[begin];
        w.block_end = (uint32_t)(idx->list_blk_base[end - 1] + idx->list_nb[end - 1]);
        std::vector<ds2i_dev::QTerm> lists;
        DS2I_TRY
        lists.resize(V);
        DS2I_CATCH
        for (uint64_t t = 0; t < V; ++t) lists[t] = ds2i_make_qterm(idx, (uint32_t)(begin + t));
        ds2i_dev::QTerm* d_lists = nullptr;
        uint64_t* d_first = nullptr;
        if (dev.alloc(&d_lists, sizeof(ds2i_dev::QTerm) * V) != hipSuccess || dev.alloc(&d_first, 8 * (V + 1)) != hipSuccess) return nomem();
        HIP_OK(hipMemcpy(d_lists, lists.data(), sizeof(ds2i_dev::QTerm) * V, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_first, offs, 8 * (V + 1), hipMemcpyHostToDevice));
        w.lists = d_lists;
        w.list_first = d_first;
        return DS2I_OK;
    }
    // a.w is set here; ms accumulates the kernel's hipEvent time. No blocks: no launch.
    template <class Args>
    int launch(const ds2i_hip_index* idx, Args& a, hipError_t (*general)(const Args&, unsigned, hipStream_t),
               hipError_t (*side)(const Args&, unsigned, hipStream_t), double& ms) const {
        if (!blocks()) return DS2I_OK;
        a.w = w;
        const unsigned grid = ds2i_walk_grid(idx, blocks());
        hipStream_t s = idx->stream[0];
        HIP_OK(timed_span(s, ms, [&] { return (idx->decode_through_side_tables() ? side : general)(a, grid, s); }));
        return DS2I_OK;
    }
};

// capi_extract.cpp. parse_image: the image on the host, as ds2i_hip_index_open reads it -- number of documents, number of lists
// and, if asked for, every list's length; a garbage image is DS2I_EFORMAT here, before a device is looked for.
// extract_to_device: the postings of lists [begin, end) of an open index into two fresh device buffers of exactly offs[end - begin]
// postings each (offs as WalkStaging::stage takes them): one launch; DS2I_ENOMEM when they do not fit beside the index.
// convert_image: an image to the image of the same postings in another kind (one of ds2i_check_encoder_kind's; the postings
// of a block codec target never leave the device): bare upload, extraction of every list, the source closed, the encoder. What ds2i_hip_convert_index does once its
// arguments are checked and the image is parsed, and what the transcoding upload does (capi.cpp, index_open_transcoded). Every
// device buffer of the attempt is released before it returns an error. no_room (may be null) is set when that error is the
// extraction's DS2I_ENOMEM: the postings do not fit beside the source image. doc_map (null: a plain conversion): a checked permutation of
// the image's documents; between the source's release and the encoder the postings are renumbered through it where they lie
// (remap_device_postings). remap_ms (may be null) then receives the hipEvent milliseconds of {map kernel, sort class 1, 2, 3,
// extraction, encoder}; device_ms is their sum.
int ds2i_parse_image(int index_kind, const void* image, size_t bytes, uint64_t& num_docs, uint64_t& nlists, std::vector<uint32_t>* lengths);
int ds2i_extract_to_device(ds2i_hip_index* idx, uint64_t begin, uint64_t end, const uint64_t* offs, DevPostings& out, double& ms);
struct ds2i_blob;
int ds2i_convert_image(const char* who, int device, int from_kind, const void* image, size_t bytes, int to_kind, ds2i_blob** out_image,
                       double* device_ms, bool* no_room, const uint32_t* doc_map = nullptr, double* remap_ms = nullptr);

// capi_remap.cpp. The postings of nlists lists on `device` (offs on the host, as WalkStaging::stage takes them) renumbered: every doc-id
// through doc_map -- a permutation of [0, num_docs), checked by the caller (ds2i_check_doc_map) -- and every list sorted again by its
// new doc-ids, the freqs with them. dp's buffers are the input and, on DS2I_OK, hold the result: they may have been exchanged for the
// sort's second pair, and whichever pair is not the result has been freed, with every table of the sort, before this returns.
// While it runs: 16 bytes per posting when a list is longer than a workgroup sorts (else 8), 4 per document, 8 per list.
// A doc-id >= num_docs among the postings is DS2I_EFORMAT (nothing is read past the map). ms[0 .. 3] receive the hipEvent
// milliseconds of the map kernel and of sort classes 1, 2 and 3. A null doc_map skips the map kernel and its 4 bytes per document: the
// postings hold their new doc-ids already (all < num_docs) and only the sort runs -- what a merge asks for (capi_merge.cpp).
int ds2i_remap_device_postings(const char* who, int device, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, DevPostings& dp,
                               const uint32_t* doc_map, double ms[4]);

// capi_encode.cpp, for capi_extract.cpp (ds2i_hip_convert_index). check_encoder_kind: DS2I_OK for the seven kinds the GPU encoder
// writes, else ds2i_hip_encode_index's DS2I_EINVAL naming them. encode_device_postings: ds2i_hip_encode_index over postings that
// lie on `device` already (list_offsets on the host); d_docs / d_freqs were hipMalloc-ed and belong to the callee from the call on,
// whatever it returns. The block codecs never bring the postings to the host; the Elias-Fano layouts bring them down once, for
// the host planner, and apply ds2i_hip_encode_index's input checks to them.
int ds2i_check_encoder_kind(const char* who, int index_kind);
int ds2i_encode_device_postings(const char* who, int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                                uint32_t* d_docs, uint32_t* d_freqs, ds2i_blob** image, double* device_ms);
// build_device_postings: the same, and from the same staging the wand_data image over doc_sizes (num_docs lengths, num_docs >= 1)
// when wand_image is not null, as ds2i_hip_build_collection makes both from one upload: every doc-id must be < num_docs. Neither output
// is written unless both succeed.
int ds2i_build_device_postings(const char* who, int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                               uint32_t* d_docs, uint32_t* d_freqs, const uint32_t* doc_sizes, ds2i_blob** image, ds2i_blob** wand_image,
                               double* device_ms);
