// HIP kernel (gfx950, wave64) of the index merge: the postings of ONE source stored where the host plan (host_merge.hpp, merge_plan) puts
// them among the merged postings.
//   k_merge_place    source posting i of source list t goes to dst_first[t] + (i - src_first[t]); its doc-id goes through the source's
//                    doc map, or has the source's base added. A doc-id at or past map_len raises a.flag and that posting is not stored:
//                    nothing is read past the map (the host refuses the result).
// A wavefront takes a window of MERGE_WINDOW consecutive source postings at a time and reads them coalesced, a posting a lane, 64 a step.
// The list of the window's first posting is found once per window, by a binary search over all of the source's offsets, and so is the
// list of its last; a lane then searches only between those two. A window inside one list (a list of millions of postings) searches
// nothing more, a window over many lists of one posting searches ten steps at the most. Wavefronts stride over the windows, so any grid
// covers any source. Every index comes from the host plan: src_first[nlists] == postings, and a run written at dst_first[t] ends where
// the plan's next run begins. Empty source lists are skipped by the search (the LAST list that starts at or before i is i's).
#include <hip/hip_runtime.h>

#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

constexpr uint32_t THREADS = 256, WAVES = THREADS / 64;
static_assert(MERGE_WINDOW % 64 == 0, "a window is whole steps of a wavefront");

// the largest t in [lo, hi] with first[t] <= i; the caller knows first[lo] <= i
__device__ __forceinline__ uint32_t list_of(const uint64_t* __restrict__ first, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(THREADS) k_merge_place(MergePlaceArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwindows = (a.postings + MERGE_WINDOW - 1) / MERGE_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * MERGE_WINDOW;
        const uint64_t w1 = w0 + MERGE_WINDOW < a.postings ? w0 + MERGE_WINDOW : a.postings;
        const uint32_t t_lo = list_of(a.src_first, 0, a.nlists - 1, w0); // (src_first[0] == 0 <= w0)
        const uint32_t t_hi = list_of(a.src_first, t_lo, a.nlists - 1, w1 - 1);
        for (uint64_t i = w0 + lane; i < w1; i += 64) {
            const uint32_t t = t_lo == t_hi ? t_lo : list_of(a.src_first, t_lo, t_hi, i);
            const uint32_t d = a.src_docs[i];
            if (d < a.map_len) {
                const uint64_t to = a.dst_first[t] + (i - a.src_first[t]);
                a.dst_docs[to] = a.doc_map ? a.doc_map[d] : a.base + d;
                a.dst_freqs[to] = a.src_freqs[i];
            } else atomicOr(a.flag, 1u);
        }
    }
}

} // namespace

extern "C" hipError_t ds2i_launch_merge_place(const MergePlaceArgs& a, unsigned grid, hipStream_t s) {
    if (!a.postings || !grid) return hipSuccess;
    if (!a.nlists) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_merge_place, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}
