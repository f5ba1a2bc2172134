// HIP kernel (gfx950, wave64) of the shard set: the top-k rows that several shards answered for the same queries merged into the rows the
// whole collection answers (include/ds2i_build.h, ds2i_merge_topk, states the semantics; host_shard.hpp holds the host twin).
//
// A candidate's key is the u64 ((0xFFFFFFFF - bits(score)) << 32) | collection doc-id: ascending key = score descending, equal scores by
// collection doc-id ascending. The order is total and made of integers, so the kernel and the twin agree element for element.
//
//   k_merge_topk   one wavefront (= one workgroup) a query; workgroups stride over the queries. Three buffers of a.pow2 keys in dynamic
//                  LDS: the best keys so far, the incoming row, and their union. Per row set: the row's keys are formed (a lane a
//                  candidate, coalesced reads of scores and docs, one gather through the doc map); a row of a set whose map is not
//                  increasing is sorted by a bitonic network over the next power of two of its length (the host marks those sets: under an
//                  increasing map a row already is in key order); then the two sorted sides are merged by rank: an element's rank in the
//                  union is its own position plus the number of elements of the other side before it -- a lower bound for the best side,
//                  an upper bound for the incoming side, so that the ranks are distinct even when keys repeat -- and elements of rank < k
//                  are stored at their rank. The union becomes the best side.
// Bounds: a length is clamped to k <= a.pow2, a local id at or past its map is not looked up (the host refuses such rows before the
// launch), every LDS store is at an index < k, every global store at q * k + i with i < k. No atomics: the result does not depend on
// scheduling. Every branch and every loop's trip count around a barrier is the same for all lanes.
#include <hip/hip_runtime.h>

#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

using u64 = unsigned long long;

__device__ __forceinline__ u64 topk_key(float score, uint32_t g) { return (u64)(0xFFFFFFFFu - __float_as_uint(score)) << 32 | g; }

__global__ void __launch_bounds__(64) k_merge_topk(MergeTopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* const buf0 = (u64*)smem;
    u64* const row = buf0 + a.pow2;
    u64* const buf2 = row + a.pow2;
    const uint32_t lane = threadIdx.x;
    const uint32_t k = a.k;
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        u64 *best = buf0, *next = buf2;
        uint32_t nbest = 0;
        const size_t base = (size_t)q * k;
        for (uint32_t r = 0; r < a.nrows; ++r) {
            const TopkRowSet rs = a.rows[r];
            uint32_t len = rs.lens[q];
            if (len > k) len = k;
            if (len == 0) continue;
            for (uint32_t i = lane; i < len; i += 64) {
                const uint32_t doc = rs.docs[base + i];
                uint32_t g = doc;
                if (rs.doc_map) g = doc < rs.map_len ? rs.doc_map[doc] : 0xFFFFFFFFu;
                row[i] = topk_key(rs.scores[base + i], g);
            }
            if (a.unsorted >> r & 1ull) {
                uint32_t n2 = 1;
                while (n2 < len) n2 <<= 1; // <= a.pow2
                for (uint32_t i = len + lane; i < n2; i += 64) row[i] = ~0ull;
                __syncthreads();
                for (uint32_t size = 2; size <= n2; size <<= 1)
                    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                        for (uint32_t t = lane; t < n2 / 2; t += 64) {
                            const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                            const bool ascending = (lo & size) == 0;
                            const u64 x = row[lo], y = row[hi];
                            if ((x > y) == ascending) {
                                row[lo] = y;
                                row[hi] = x;
                            }
                        }
                        __syncthreads();
                    }
            } else {
                __syncthreads();
            }
            // the union by rank: best before row on equal keys
            for (uint32_t i = lane; i < nbest; i += 64) {
                const u64 key = best[i];
                uint32_t lo = 0, hi = len;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (row[mid] < key) lo = mid + 1; else hi = mid;
                }
                if (i + lo < k) next[i + lo] = key;
            }
            for (uint32_t j = lane; j < len; j += 64) {
                const u64 key = row[j];
                uint32_t lo = 0, hi = nbest;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (best[mid] <= key) lo = mid + 1; else hi = mid;
                }
                if (j + lo < k) next[j + lo] = key;
            }
            __syncthreads();
            u64* const t = best;
            best = next;
            next = t;
            nbest = nbest + len < k ? nbest + len : k;
        }
        for (uint32_t i = lane; i < k; i += 64) {
            const bool have = i < nbest;
            const u64 key = have ? best[i] : 0;
            a.out_scores[base + i] = have ? __uint_as_float(0xFFFFFFFFu - (uint32_t)(key >> 32)) : -__builtin_inff();
            a.out_docs[base + i] = have ? (uint32_t)key : 0xFFFFFFFFu;
        }
        if (lane == 0) a.out_lens[q] = nbest;
        __syncthreads();
    }
}

} // namespace

extern "C" uint32_t ds2i_hip_merge_topk_grid(uint32_t compute_units, uint32_t k) { return merge_topk_grid(~0ull >> 1, (int)compute_units, k); }

extern "C" hipError_t ds2i_launch_merge_topk(const MergeTopkArgs& a, unsigned grid, hipStream_t s) {
    if (!a.nq || !grid) return hipSuccess;
    if (a.k == 0 || a.k > MERGE_TOPK_MAX_K || a.pow2 < a.k || a.pow2 > MERGE_TOPK_MAX_K || (a.pow2 & (a.pow2 - 1)) || a.pow2 < 2 ||
        a.nrows > MERGE_TOPK_MAX_ROWS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_merge_topk, dim3(grid), dim3(64), 24 * (size_t)a.pow2, s, a);
    return hipGetLastError();
}
