// the opt layout's partition end points as the four blobs of ds2i_opt_partition (ds2i_build.h) / ds2i_hip_opt_partition (ds2i_hip.h):
// per side the u32 end points of all lists back to back and nlists + 1 u64 offsets into them. No output is written unless all are.
#pragma once
#include <memory>

#include "capi_blob.hpp"
#include "host_freq_plan.hpp"

inline void partition_blobs(const ds2i_host::opt_partitions& parts, ds2i_blob** docs_ends, ds2i_blob** docs_offs, ds2i_blob** freqs_ends,
                            ds2i_blob** freqs_offs) {
    std::unique_ptr<ds2i_blob> b[4];
    for (int side = 0; side < 2; ++side) {
        b[2 * side].reset(new ds2i_blob);
        b[2 * side + 1].reset(new ds2i_blob);
        const uint8_t* p = (const uint8_t*)parts.ends[side].data();
        b[2 * side]->data.assign(p, p + 4 * parts.ends[side].size());
        p = (const uint8_t*)parts.offs[side].data();
        b[2 * side + 1]->data.assign(p, p + 8 * parts.offs[side].size());
    }
    *docs_ends = b[0].release();
    *docs_offs = b[1].release();
    *freqs_ends = b[2].release();
    *freqs_offs = b[3].release();
}
