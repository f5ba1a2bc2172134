// HIP kernels (gfx950, wave64) that ORDER the documents of a collection by recursive graph bisection (capi_order.cpp launches them;
// abi_structs.hpp: OrderArgs; order_cost.hpp: the arithmetic, shared with the host twin host_order.hpp, which states the algorithm).
// Everything here is integer arithmetic, and every sum that atomics build is a sum of integers, so the result does not depend on the
// order in which anything ran: the device returns the twin's map and trace element for element.
//
// The layout. The lists lie on the device as entries: a.docs[i] is the p0 (the position at the level's start) of posting i's document,
// and every list is in p0 order: at level 0 that is the input (p0 = doc-id), at every later level the entries go through the previous
// level's inverse (k_order_renumber) and the segmented sort of the remap puts every list in order again. So a term's documents of one
// level segment are one RUN of consecutive entries, and the two degrees of (term, segment) live at the run's first entry, its HEAD.
// No forward index is built and no float is touched.
//   k_order_check      a doc-id at or past num_docs raises a.flag (the host refuses: nothing later indexes a table by an unchecked id)
//   k_order_renumber   docs[i] = inv[docs[i]]: the entries named by the new level's p0
//   k_order_level      per position s: half_of[s] (the level l + 1 segment of s, one 64-bit division), side[s] = its low bit,
//                      members[s] = s
//   k_order_runs       once a level, per entry: its list (as invert_kernels.hip finds a row: two searches per window, one per lane
//                      between them), then two binary searches in its own list for the segment's two bounds: back[i] = i - head, and at
//                      the head run_len = the run's entries
//   k_order_degrees    once an iteration: deg_right[head] += side[p0]. The entries of a run are consecutive, so within a wavefront the
//                      lanes of one run are consecutive too: the first of them adds the popcount of their side bits, one atomic per
//                      (run, wavefront step) that has a document on the right, instead of one per entry
//   k_order_gains      per entry: dl and dr from the head, order_term_cost, and a 64-bit integer atomicAdd into gain[p0]
//   k_order_keys       per slot: keys[s] = the order-reversing image of the clamped gain of members[s]; (keys, members) is the pair the
//                      segmented sort takes, the 2^(l+1) halves its segments
//   k_order_presort_keys  keys[s] = members[s]: the pair sorted by p0 first, where a half is longer than a workgroup sorts and the
//                      sort by gain is only stable (LSD: p0, then gain)
//   k_order_swap       per left slot l0 + i with a partner r0 + i: gains from the two keys, the test gain_left + gain_right > 0, the
//                      exchange of the two members and their side bits. A pair belongs to one thread, so nothing races; the exchanges
//                      of a wavefront are counted with a ballot and added once
//   k_order_compose    at a level's end: next_order[s] = order[members[s]], inv[members[s]] = s
//   k_order_finish     doc_map[order[s]] = s
// No kernel waits for another workgroup. Every index that comes from data (a p0, a member, a degree) is compared with its bound before
// it is used; after a clean check kernel none of those comparisons fails. Every loop with a ballot has the same trip count in all lanes.
#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "order_cost.hpp"

using namespace ds2i_dev;
using namespace ds2i_host;

namespace {

constexpr uint32_t THREADS = SPLIT_THREADS, WAVES = THREADS / 64;
static_assert(ORDER_WINDOW % 64 == 0, "a window is whole steps of a wavefront");

// the largest t in [lo, hi] with first[t] <= i; the caller knows first[lo] <= i. Empty lists are skipped.
__device__ __forceinline__ uint32_t list_of(const uint64_t* __restrict__ first, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// the first position in [lo, hi) whose entry is >= bound, or hi
__device__ __forceinline__ uint64_t first_at_or_above(const uint32_t* __restrict__ docs, uint64_t lo, uint64_t hi, uint64_t bound) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (docs[mid] < bound) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(THREADS) k_order_check(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < a.postings; i += stride)
        if (a.docs[i] >= a.num_docs) atomicOr(a.flag, 1u);
}

__global__ void __launch_bounds__(THREADS) k_order_renumber(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < a.postings; i += stride) {
        const uint32_t p = a.docs[i];
        if (p < a.num_docs) a.docs[i] = a.inv[p];
    }
}

__global__ void __launch_bounds__(THREADS) k_order_level(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x; s < a.num_docs; s += stride) {
        const uint32_t h = order_segment_of(a.num_docs, a.level + 1, s);
        a.half_of[s] = h;
        a.side[s] = h & 1u;
        a.members[s] = (uint32_t)s;
    }
}

__global__ void __launch_bounds__(THREADS) k_order_runs(OrderArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwindows = (a.postings + ORDER_WINDOW - 1) / ORDER_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * ORDER_WINDOW;
        const uint64_t w1 = w0 + ORDER_WINDOW < a.postings ? w0 + ORDER_WINDOW : a.postings;
        const uint32_t t_lo = list_of(a.list_first, 0, a.nlists - 1, w0); // (list_first[0] == 0 <= w0)
        const uint32_t t_hi = list_of(a.list_first, t_lo, a.nlists - 1, w1 - 1);
        for (uint64_t i = w0 + lane; i < w1; i += 64) {
            const uint32_t t = t_lo == t_hi ? t_lo : list_of(a.list_first, t_lo, t_hi, i);
            const uint64_t first = a.list_first[t], end = a.list_first[t + 1];
            const uint32_t p = a.docs[i];
            uint64_t head = i, len = 1;
            if (p < a.num_docs && first <= i && i < end) {
                const uint32_t seg = a.half_of[p] >> 1;
                head = first_at_or_above(a.docs, first, i, order_bound(a.num_docs, a.level, seg)); // (docs[i] >= the bound: head <= i)
                if (head == i) len = first_at_or_above(a.docs, i + 1, end, order_bound(a.num_docs, a.level, (uint64_t)seg + 1)) - i;
            }
            a.back[i] = (uint32_t)(i - head); // (a list holds fewer than 2^32 entries)
            if (head == i) a.run_len[i] = (uint32_t)len;
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_order_degrees(OrderArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwindows = (a.postings + ORDER_WINDOW - 1) / ORDER_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    const uint64_t above = lane == 63u ? 0ull : ~0ull << (lane + 1); // the lanes above this one
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * ORDER_WINDOW;
        const uint64_t w1 = w0 + ORDER_WINDOW < a.postings ? w0 + ORDER_WINDOW : a.postings;
        for (uint64_t i0 = w0; i0 < w1; i0 += 64) {
            const uint64_t i = i0 + lane;
            const bool valid = i < w1;
            const uint32_t back = valid ? a.back[i] : 0u;
            const uint32_t p = valid ? a.docs[i] : 0u;
            const bool right = valid && p < a.num_docs && a.side[p] != 0u;
            // a lane leads the lanes of its run in this step: the wavefront's first lane, or a head
            const bool leader = valid && (lane == 0 || back == 0);
            const uint64_t leaders = __ballot(leader), rights = __ballot(right);
            if (leader) {
                const uint64_t later = leaders & above;
                const uint64_t mine = later ? ((1ull << (__ffsll((unsigned long long)later) - 1)) - 1) & ~((1ull << lane) - 1) : ~((1ull << lane) - 1);
                const uint32_t count = (uint32_t)__popcll(rights & mine);
                if (count && back <= i) atomicAdd(&a.deg_right[i - back], count);
            }
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_order_gains(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < a.postings; i += stride) {
        const uint32_t p = a.docs[i], back = a.back[i];
        if (p >= a.num_docs || back > i) continue;
        const uint64_t head = i - back;
        const uint32_t len = a.run_len[head], dr = a.deg_right[head];
        if (len > a.num_docs || dr > len) continue;
        const uint32_t side = a.side[p], seg = a.half_of[p] >> 1;
        const uint64_t b0 = order_bound(a.num_docs, a.level + 1, 2ull * seg), b1 = order_bound(a.num_docs, a.level + 1, 2ull * seg + 1),
                       b2 = order_bound(a.num_docs, a.level + 1, 2ull * seg + 2);
        const uint32_t nl = (uint32_t)(b1 - b0), nr = (uint32_t)(b2 - b1), dl = len - dr;
        const int64_t c = side ? order_term_cost(a.logq, nr, nl, dr, dl) : order_term_cost(a.logq, nl, nr, dl, dr);
        atomicAdd(&a.gain[p], (unsigned long long)c);
    }
}

__global__ void __launch_bounds__(THREADS) k_order_keys(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x; s < a.num_docs; s += stride) {
        const uint32_t p = a.members[s];
        a.keys[s] = p < a.num_docs ? order_gain_key(order_clamp_gain((int64_t)a.gain[p])) : ~0u;
    }
}

__global__ void __launch_bounds__(THREADS) k_order_presort_keys(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x; s < a.num_docs; s += stride) a.keys[s] = a.members[s];
}

__global__ void __launch_bounds__(THREADS) k_order_swap(OrderArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    uint32_t count = 0;
    for (uint64_t s0 = (uint64_t)blockIdx.x * THREADS + (threadIdx.x & ~63u); s0 < a.num_docs; s0 += stride) { // (s0: the same in all lanes)
        const uint64_t s = s0 + lane;
        bool exchanged = false;
        if (s < a.num_docs) {
            const uint32_t h = a.half_of[s];
            if (!(h & 1u)) { // a left slot: it owns the pair
                const uint64_t l0 = order_bound(a.num_docs, a.level + 1, h), r0 = order_bound(a.num_docs, a.level + 1, (uint64_t)h + 1),
                               r1 = order_bound(a.num_docs, a.level + 1, (uint64_t)h + 2);
                const uint64_t partner = r0 + (s - l0);
                if (s >= l0 && partner < r1 && partner < a.num_docs) {
                    const int64_t sum = (int64_t)order_key_gain(a.keys[s]) + (int64_t)order_key_gain(a.keys[partner]);
                    const uint32_t pl = a.members[s], pr = a.members[partner];
                    if (sum > 0 && pl < a.num_docs && pr < a.num_docs) {
                        a.members[s] = pr;
                        a.members[partner] = pl;
                        a.side[pl] = 1u;
                        a.side[pr] = 0u;
                        exchanged = true;
                    }
                }
            }
        }
        count += (uint32_t)__popcll(__ballot(exchanged));
    }
    if (lane == 0 && count) atomicAdd(a.exchanges, (unsigned long long)count);
}

__global__ void __launch_bounds__(THREADS) k_order_compose(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x; s < a.num_docs; s += stride) {
        const uint32_t p = a.members[s];
        if (p >= a.num_docs) continue;
        a.next_order[s] = a.order[p];
        a.inv[p] = (uint32_t)s;
    }
}

__global__ void __launch_bounds__(THREADS) k_order_finish(OrderArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x; s < a.num_docs; s += stride) {
        const uint32_t d = a.order[s];
        if (d < a.num_docs) a.doc_map[d] = (uint32_t)s;
    }
}

} // namespace

#define DS2I_ORDER_LAUNCHER(name, kernel, nonempty)                                      \
    extern "C" hipError_t name(const OrderArgs& a, unsigned grid, hipStream_t s) {      \
        if (!(nonempty) || !grid) return hipSuccess;                                     \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), 0, s, a);                  \
        return hipGetLastError();                                                        \
    }
DS2I_ORDER_LAUNCHER(ds2i_launch_order_check, k_order_check, a.postings)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_renumber, k_order_renumber, a.postings)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_level, k_order_level, a.num_docs)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_runs, k_order_runs, a.postings && a.nlists)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_degrees, k_order_degrees, a.postings)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_gains, k_order_gains, a.postings)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_keys, k_order_keys, a.num_docs)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_presort_keys, k_order_presort_keys, a.num_docs)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_swap, k_order_swap, a.num_docs)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_compose, k_order_compose, a.num_docs)
DS2I_ORDER_LAUNCHER(ds2i_launch_order_finish, k_order_finish, a.num_docs)
#undef DS2I_ORDER_LAUNCHER
