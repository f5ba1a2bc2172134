// HIP kernels (gfx950, wave64) that RENUMBER the documents of a staged collection: every doc-id goes through a doc-id map, and every list is
// sorted again by its new doc-ids, the freqs travelling with them. The keys of one list are distinct (the map is a permutation), so the
// sorted list is unique whatever the algorithm; a posting is the 64-bit pair (doc-id << 32 | freq) and pairs are compared whole.
//   k_remap_map      docs[i] = doc_map[docs[i]], grid-stride. A doc-id outside the map raises a.flag and is left alone: nothing is read
//                    past the map (the host refuses the result).
// The sort, planned on the host from the list lengths (capi_remap.cpp, plan_sort; abi_structs.hpp, RemapArgs):
//   k_remap_sort1    class 1, n <= REMAP_W: one WAVEFRONT per list, a posting per lane, a bitonic network over the smallest power of two
//                    that holds the list, through __shfl_xor (DPP / ds_bpermute); lanes past the list hold the all-ones pair, which no
//                    posting equals (a doc-id is < num_docs <= 2^32 - 1) and which sorts behind every posting. Waves stride over the class.
//   k_remap_sort2    class 2, n <= REMAP_L: one WORKGROUP per list, the pairs in LDS, the same network with a barrier a step.
//                    Workgroups stride over the class.
//   class 3, longer lists, all of them together, cut into tiles of at most REMAP_T postings of one list: an LSD radix sort, REMAP_DIGIT
//   bits a pass over the key bits num_docs needs, between two buffer pairs. One pass is three launches on one stream:
//   k_remap_hist     a workgroup per tile (striding): the tile's digit counts, one word per digit, to a.hist
//   k_remap_scan     a workgroup per list, a thread per digit: a.hist turned in place into where each (digit, tile) run starts
//                    within the list -- digit-major, tile-minor, from 0 for every list
//   k_remap_scatter  a workgroup per tile (striding): the tile walked 256 postings at a time in order; a posting's place is its run's
//                    start + the postings of its digit in the chunks, waves and lanes before it (ballots within the wave, a count
//                    per wave and digit in LDS across waves), so equal digits keep their order: what LSD needs between passes.
// No kernel waits for another workgroup: what one launch wrote the next one reads, and the kernel boundary is the only ordering.
// Every loop bound and index comes from the host plan or from list_first; a ragged last tile or chunk is masked, never padded with a
// neighbour's postings. Class 1 and 2 read a list whole before they write it, so they may write where they read (out == in).
#include <hip/hip_runtime.h>

#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

constexpr uint32_t THREADS = 256, WAVES = THREADS / 64, NDIGITS = 1u << REMAP_DIGIT;
static_assert(NDIGITS == THREADS, "the radix kernels keep one digit per thread");
static_assert((REMAP_L & (REMAP_L - 1)) == 0 && REMAP_W == 64, "class bounds: a wavefront, a power of two");
constexpr unsigned long long PAD = ~0ull;

__device__ __forceinline__ unsigned long long pack(uint32_t doc, uint32_t freq) { return (unsigned long long)doc << 32 | freq; }
// the element a compare-exchange step leaves at position `i` of pair (i, i ^ j) inside the k-block of a bitonic network
__device__ __forceinline__ unsigned long long keep(unsigned long long mine, unsigned long long other, uint32_t i, uint32_t k, uint32_t j) {
    const bool ascending = (i & k) == 0, lower = (i & j) == 0;
    const bool smaller = mine < other;
    return (lower == ascending) == smaller ? mine : other;
}

__global__ void __launch_bounds__(THREADS) k_remap_map(RemapArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < a.postings; i += stride) {
        const uint32_t d = a.docs[i];
        if (d < a.num_docs) a.docs[i] = a.doc_map[d];
        else atomicOr(a.flag, 1u);
    }
}

__global__ void __launch_bounds__(THREADS) k_remap_sort1(RemapArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * WAVES;
    for (uint32_t w = blockIdx.x * WAVES + (threadIdx.x >> 6); w < a.nlists1; w += nwaves) {
        const uint32_t t = a.lists1[w];
        const uint64_t first = a.list_first[t];
        const uint64_t len = a.list_first[t + 1] - first;
        const uint32_t n = len < REMAP_W ? (uint32_t)len : REMAP_W; // (the plan puts no longer list here)
        const bool valid = lane < n;
        unsigned long long v = valid ? pack(a.docs[first + lane], a.freqs[first + lane]) : PAD;
        for (uint32_t k = 2; (k >> 1) < n; k <<= 1)
            for (uint32_t j = k >> 1; j; j >>= 1) v = keep(v, __shfl_xor(v, (int)j), lane, k, j);
        if (valid) {
            a.out_docs[first + lane] = (uint32_t)(v >> 32);
            a.out_freqs[first + lane] = (uint32_t)v;
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_remap_sort2(RemapArgs a) {
    __shared__ unsigned long long s[REMAP_L];
    const uint32_t tid = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < a.nlists2; b += gridDim.x) {
        const uint32_t t = a.lists2[b];
        const uint64_t first = a.list_first[t];
        const uint64_t len = a.list_first[t + 1] - first;
        const uint32_t n = len < REMAP_L ? (uint32_t)len : REMAP_L; // (the plan puts no longer list here)
        uint32_t size = 1;
        while (size < n) size <<= 1; // <= REMAP_L, a power of two
        for (uint32_t p = tid; p < size; p += THREADS) s[p] = p < n ? pack(a.docs[first + p], a.freqs[first + p]) : PAD;
        __syncthreads();
        for (uint32_t k = 2; k <= size; k <<= 1)
            for (uint32_t j = k >> 1; j; j >>= 1) {
                for (uint32_t q = tid; q < size / 2; q += THREADS) {
                    const uint32_t lo = 2 * j * (q / j) + q % j, hi = lo + j;
                    const unsigned long long x = s[lo], y = s[hi];
                    s[lo] = keep(x, y, lo, k, j);
                    s[hi] = keep(y, x, hi, k, j);
                }
                __syncthreads();
            }
        for (uint32_t p = tid; p < n; p += THREADS) {
            a.out_docs[first + p] = (uint32_t)(s[p] >> 32);
            a.out_freqs[first + p] = (uint32_t)s[p];
        }
        __syncthreads(); // (the next list overwrites s)
    }
}

__global__ void __launch_bounds__(THREADS) k_remap_hist(RemapArgs a, const uint32_t* __restrict__ src, uint32_t shift) {
    __shared__ uint32_t h[NDIGITS];
    const uint32_t tid = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const RemapTile T = a.tiles[tile];
        h[tid] = 0;
        __syncthreads();
        for (uint32_t p = tid; p < T.count; p += THREADS) atomicAdd(&h[(src[T.first + p] >> shift) & (NDIGITS - 1)], 1u);
        __syncthreads();
        a.hist[(uint64_t)tile * NDIGITS + tid] = h[tid];
    }
}

__global__ void __launch_bounds__(THREADS) k_remap_scan(RemapArgs a) {
    __shared__ uint32_t total[NDIGITS];
    const uint32_t d = threadIdx.x;
    const RemapLong L = a.longs[blockIdx.x];
    uint32_t* const h = a.hist + (uint64_t)L.tile0 * NDIGITS + d;
    uint32_t sum = 0;
    for (uint32_t t = 0; t < L.ntiles; ++t) sum += h[(uint64_t)t * NDIGITS];
    total[d] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t e = 0; e < d; ++e) run += total[e];
    for (uint32_t t = 0; t < L.ntiles; ++t) {
        const uint32_t c = h[(uint64_t)t * NDIGITS];
        h[(uint64_t)t * NDIGITS] = run;
        run += c;
    }
}

__global__ void __launch_bounds__(THREADS) k_remap_scatter(RemapArgs a, const uint32_t* __restrict__ src_docs, const uint32_t* __restrict__ src_freqs,
                                                           uint32_t* __restrict__ dst_docs, uint32_t* __restrict__ dst_freqs, uint32_t shift) {
    __shared__ uint32_t base[NDIGITS];         // where the next posting of each digit goes within the list
    __shared__ uint32_t wcount[WAVES][NDIGITS]; // this chunk: postings per wave and digit
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const RemapTile T = a.tiles[tile];
        const uint64_t list_first = a.longs[T.list3].first;
        base[tid] = a.hist[(uint64_t)tile * NDIGITS + tid];
        for (uint32_t w = 0; w < WAVES; ++w) wcount[w][tid] = 0;
        __syncthreads();
        for (uint32_t c0 = 0; c0 < T.count; c0 += THREADS) {
            const uint32_t p = c0 + tid;
            const bool valid = p < T.count;
            const uint32_t key = valid ? src_docs[T.first + p] : 0u;
            const uint32_t freq = valid ? src_freqs[T.first + p] : 0u;
            const uint32_t digit = (key >> shift) & (NDIGITS - 1);
            unsigned long long same = __ballot(valid); // the wave's valid lanes that hold my digit
            for (uint32_t b = 0; b < REMAP_DIGIT; ++b) {
                const bool bit = (digit >> b) & 1u;
                const unsigned long long set = __ballot(bit);
                same &= bit ? set : ~set;
            }
            const uint32_t rank = (uint32_t)__popcll(same & below);
            if (valid && rank == 0) wcount[wave][digit] = (uint32_t)__popcll(same);
            __syncthreads();
            if (valid) {
                uint32_t pos = base[digit] + rank;
                for (uint32_t w = 0; w < wave; ++w) pos += wcount[w][digit];
                dst_docs[list_first + pos] = key;
                dst_freqs[list_first + pos] = freq;
            }
            __syncthreads();
            uint32_t chunk = 0;
            for (uint32_t w = 0; w < WAVES; ++w) {
                chunk += wcount[w][tid];
                wcount[w][tid] = 0;
            }
            base[tid] += chunk;
            __syncthreads();
        }
    }
}

} // namespace

extern "C" void ds2i_hip_remap_class_bounds(uint32_t bounds[3]) {
    if (!bounds) return;
    bounds[0] = REMAP_W;
    bounds[1] = REMAP_L;
    bounds[2] = REMAP_T;
}

extern "C" hipError_t ds2i_launch_remap_map(const RemapArgs& a, unsigned grid, hipStream_t s) {
    if (!a.postings || !grid) return hipSuccess;
    hipLaunchKernelGGL(k_remap_map, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_remap_sort1(const RemapArgs& a, unsigned grid, hipStream_t s) {
    if (!a.nlists1 || !grid) return hipSuccess;
    hipLaunchKernelGGL(k_remap_sort1, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_remap_sort2(const RemapArgs& a, unsigned grid, hipStream_t s) {
    if (!a.nlists2 || !grid) return hipSuccess;
    hipLaunchKernelGGL(k_remap_sort2, dim3(grid), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_remap_radix_pass(const RemapArgs& a, int from_second, uint32_t shift, unsigned grid, hipStream_t s) {
    if (!a.ntiles || !grid) return hipSuccess;
    if (!a.docs_b || !a.freqs_b || !a.hist || shift >= 32) return hipErrorInvalidValue;
    const uint32_t *src_docs = from_second ? a.docs_b : a.docs, *src_freqs = from_second ? a.freqs_b : a.freqs;
    uint32_t *dst_docs = from_second ? a.docs : a.docs_b, *dst_freqs = from_second ? a.freqs : a.freqs_b;
    hipLaunchKernelGGL(k_remap_hist, dim3(grid), dim3(THREADS), 0, s, a, src_docs, shift);
    hipLaunchKernelGGL(k_remap_scan, dim3(a.nlongs), dim3(THREADS), 0, s, a);
    hipLaunchKernelGGL(k_remap_scatter, dim3(grid), dim3(THREADS), 0, s, a, src_docs, src_freqs, dst_docs, dst_freqs, shift);
    return hipGetLastError();
}
