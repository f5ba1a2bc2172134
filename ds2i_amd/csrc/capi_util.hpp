// What the build-side C-ABI units share (capi.cpp: upload; capi_encode.cpp: encoders, wand data, optimiser; capi_verify.cpp): device
// temporaries, the timed span around a launch, the device check. (The exception guard is capi_error.hpp's DS2I_TRY / DS2I_CATCH,
// which the HIP-free capi_build.cpp uses too.)
#pragma once
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

// capi_encode.cpp, for capi_extract.cpp (ds2i_hip_convert_index). check_encoder_kind: DS2I_OK for the seven kinds the GPU encoder
// writes, else ds2i_hip_encode_index's DS2I_EINVAL naming them. encode_device_postings: ds2i_hip_encode_index over postings that
// lie on `device` already (list_offsets on the host); d_docs / d_freqs were hipMalloc-ed and belong to the callee from the call on,
// whatever it returns. The block codecs never bring the postings to the host; the Elias-Fano layouts bring them down once, for
// the host planner, and apply ds2i_hip_encode_index's input checks to them.
struct ds2i_blob;
int ds2i_check_encoder_kind(const char* who, int index_kind);
int ds2i_encode_device_postings(const char* who, int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                                uint32_t* d_docs, uint32_t* d_freqs, ds2i_blob** image, double* device_ms);
