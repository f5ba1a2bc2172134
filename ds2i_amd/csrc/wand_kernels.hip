// HIP kernel (gfx950, wave64) of the wand_data build side (create_wand_data.cpp:8-29, wand_data.hpp:20-52):
//   max_term_weight[t] = max over list t's postings of bm25::doc_term_weight(freq, norm_len[doc])
// over the CSR staging the index encoder uses (capi_encode.cpp EncStage). One wavefront per 128-posting block: two
// postings per lane, the gather of norm_len[doc], the scoring code's own doc_term_weight (device_enum.hpp, through
// device_score.hpp; -ffp-contract=off like every unit), a wave maximum, and ONE integer atomicMax per block into the
// list's slot -- the weights are non-negative floats, whose bit patterns order like their values. A maximum does not
// depend on the order of its operands, so the result is the host's (host_index.hpp list_max_weight) bit for bit at any
// grid: a list of two million postings spreads over as many waves as it has blocks, sixty thousand one-block lists
// take one wave each.
#include <hip/hip_runtime.h>

#include "device_score.hpp"
#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

struct WandArgs {
    const uint32_t* docs;      // postings of all lists, concatenated
    const uint32_t* freqs;
    const uint64_t* list_in;   // nlists + 1 posting offsets
    const uint32_t* blk_list;  // per block: its list
    const uint32_t* list_blk0; // per list: its first block (global numbering)
    const float* norm_lens;    // num_docs
    unsigned int* list_max;    // per list: bits of the largest weight so far (zeroed before the launch: +0.0f)
    uint64_t num_docs;
    uint32_t nblocks;
};

constexpr uint32_t WAND_WAVES = 4; // waves per workgroup, a block of postings each

// as list_max_weight folds: mx = max(mx, w) from 0, which also keeps a NaN (an all-empty collection's norm_len) out
DS2I_DEV float fold_max(float mx, float w) { return mx < w ? w : mx; }

__global__ void __launch_bounds__(64 * WAND_WAVES) k_wand_list_max(WandArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    for (uint64_t blk = (uint64_t)blockIdx.x * WAND_WAVES + wave; blk < a.nblocks; blk += (uint64_t)gridDim.x * WAND_WAVES) {
        const uint32_t t = a.blk_list[blk];
        const uint32_t lb = (uint32_t)blk - a.list_blk0[t];
        const uint64_t in0 = a.list_in[t];
        const uint64_t n = a.list_in[t + 1] - in0;
        const uint64_t k0 = in0 + 128ull * lb;
        const uint64_t left = n - 128ull * lb;
        const uint32_t sz = left < 128u ? (uint32_t)left : 128u;
        float mx = 0.f;
#pragma unroll
        for (uint32_t half = 0; half < 2; ++half) {
            const uint32_t i = lane + 64u * half;
            if (i < sz) {
                const uint32_t d = a.docs[k0 + i];
                // (the entry points refuse a doc-id >= num_docs on the host; the guard keeps the gather inside norm_lens regardless)
                if (d < a.num_docs) mx = fold_max(mx, doc_term_weight(a.freqs[k0 + i], a.norm_lens[d]));
            }
        }
        for (int o = 32; o; o >>= 1) mx = fold_max(mx, __shfl_xor(mx, o));
        if (lane == 0) atomicMax(a.list_max + t, __float_as_uint(mx));
    }
}

} // namespace

extern "C" hipError_t ds2i_launch_wand_list_max(const uint32_t* docs, const uint32_t* freqs, const uint64_t* list_in, const uint32_t* blk_list,
                                                const uint32_t* list_blk0, uint32_t nblocks, const float* norm_lens, uint64_t num_docs,
                                                unsigned int* list_max, unsigned max_groups, hipStream_t s) {
    WandArgs a;
    a.docs = docs;
    a.freqs = freqs;
    a.list_in = list_in;
    a.blk_list = blk_list;
    a.list_blk0 = list_blk0;
    a.norm_lens = norm_lens;
    a.list_max = list_max;
    a.num_docs = num_docs;
    a.nblocks = nblocks;
    unsigned grid = (nblocks + WAND_WAVES - 1) / WAND_WAVES;
    if (grid > max_groups) grid = max_groups;
    if (!grid) grid = 1;
    hipLaunchKernelGGL(k_wand_list_max, dim3(grid), dim3(64 * WAND_WAVES), 0, s, a);
    return hipGetLastError();
}
