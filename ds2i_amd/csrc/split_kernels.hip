// HIP kernels (gfx950, wave64) of the index split: ONE shard cut out of the source postings. The shard's postings array is the stable
// compaction of the source postings array by the flag shard_of[doc-id] == shard; a source list that keeps nothing vanishes, so no kernel
// looks for a posting's list and none needs an atomic per list. The source is cut into windows of SPLIT_WINDOW consecutive postings.
//   k_split_count    per window, the postings kept: a ballot and a popcount per step of 64 postings. A doc-id at or past num_docs raises
//                    a.flag and is not kept: shard_of is never read at or past num_docs (the host refuses the result).
//   (the host scans the window counts into u64: a.win_base, windows + 1 values)
//   k_split_offsets  per source list start i = src_first[t], the kept postings before i: win_base of i's window plus a ballot count
//                    over the window's postings before i. A wavefront a list start. The host drops the lists whose two consecutive
//                    values are equal.
//   k_split_scatter  a wavefront walks a window with a running position that starts at the window's win_base; a kept posting goes to
//                    running + popcount(ballot & lanes below), its doc-id replaced by a.local[doc-id], its freq beside it.
// The three kernels evaluate the same flag over the same postings, so the scatter's positions are the ones the count announced: every
// store lies below win_base[windows], the size of the shard's buffers (the scatter checks it all the same). All reads of the postings
// are coalesced, a posting a lane, 64 a step; every loop's trip count is the same for all lanes of a wavefront, so every ballot sees
// the whole wavefront. Wavefronts stride over the windows (or the list starts), so any grid covers any input.
#include <hip/hip_runtime.h>

#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

constexpr uint32_t THREADS = SPLIT_THREADS, WAVES = THREADS / 64;
static_assert(SPLIT_WINDOW % 64 == 0, "a window is whole steps of a wavefront");

// this lane's posting i of [.., end) is kept; `flag` (null: do not report) is raised for a doc-id outside the documents
__device__ __forceinline__ bool kept(const SplitArgs& a, uint64_t i, uint64_t end, uint32_t* flag, uint32_t& doc) {
    if (i >= end) return false;
    doc = a.src_docs[i];
    if (doc >= a.num_docs) {
        if (flag) atomicOr(flag, 1u);
        return false;
    }
    return a.shard_of[doc] == a.shard;
}

__global__ void __launch_bounds__(THREADS) k_split_count(SplitArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwindows = (a.postings + SPLIT_WINDOW - 1) / SPLIT_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * SPLIT_WINDOW;
        const uint64_t w1 = w0 + SPLIT_WINDOW < a.postings ? w0 + SPLIT_WINDOW : a.postings;
        uint32_t count = 0, doc = 0;
        for (uint64_t i0 = w0; i0 < w1; i0 += 64) count += (uint32_t)__popcll(__ballot(kept(a, i0 + lane, w1, a.flag, doc)));
        if (lane == 0) a.win_count[w] = count;
    }
}

__global__ void __launch_bounds__(THREADS) k_split_offsets(SplitArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t t = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); t < a.nstarts; t += nwaves) {
        const uint64_t i = a.src_first[t] < a.postings ? a.src_first[t] : a.postings; // (the host checked the offsets: i <= postings)
        const uint64_t w = i / SPLIT_WINDOW; // (i == postings on a window boundary: w == windows, whose win_base is the total)
        uint32_t count = 0, doc = 0;
        for (uint64_t i0 = w * SPLIT_WINDOW; i0 < i; i0 += 64) count += (uint32_t)__popcll(__ballot(kept(a, i0 + lane, i, nullptr, doc)));
        if (lane == 0) a.kept_before[t] = a.win_base[w] + count;
    }
}

__global__ void __launch_bounds__(THREADS) k_split_scatter(SplitArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1;
    const uint64_t nwindows = (a.postings + SPLIT_WINDOW - 1) / SPLIT_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    const uint64_t total = a.win_base[nwindows];
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * SPLIT_WINDOW;
        const uint64_t w1 = w0 + SPLIT_WINDOW < a.postings ? w0 + SPLIT_WINDOW : a.postings;
        uint64_t running = a.win_base[w];
        for (uint64_t i0 = w0; i0 < w1; i0 += 64) {
            uint32_t doc = 0;
            const bool keep = kept(a, i0 + lane, w1, nullptr, doc);
            const uint64_t mask = __ballot(keep);
            const uint64_t to = running + (uint32_t)__popcll(mask & below);
            if (keep && to < total) {
                a.dst_docs[to] = a.local[doc];
                a.dst_freqs[to] = a.src_freqs[i0 + lane];
            }
            running += (uint32_t)__popcll(mask);
        }
    }
}

} // namespace

extern "C" uint32_t ds2i_hip_split_window(void) { return SPLIT_WINDOW; }
extern "C" uint32_t ds2i_hip_split_grid_waves(uint32_t compute_units) { return WAVES * split_grid(~0ull >> 1, (int)compute_units); }

extern "C" hipError_t ds2i_launch_split_count(const SplitArgs& a, unsigned grid, hipStream_t s) {
    if (!a.postings || !grid) return hipSuccess;
    hipLaunchKernelGGL(k_split_count, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_split_offsets(const SplitArgs& a, unsigned grid, hipStream_t s) {
    if (!a.nstarts || !grid) return hipSuccess;
    hipLaunchKernelGGL(k_split_offsets, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_split_scatter(const SplitArgs& a, unsigned grid, hipStream_t s) {
    if (!a.postings || !grid) return hipSuccess;
    hipLaunchKernelGGL(k_split_scatter, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}
