// HIP kernels (gfx950, wave64) that PLAN the opt layout: the partition end points of partitioned_sequence, i.e. optimal_partition of
// host_pef.hpp (reference optimal_partition.hpp:67-121) for every list and both sides (docs: the doc-ids over num_docs; freqs: the
// strict prefix sums over occurrences + 1). The end points are the host's, element for element: the image built from them is the
// host builder's.
//   k_partition_plan    one WAVEFRONT per (list, side); lane c is cost class c (budget[c], computed on the host). The positions i
//                       are taken in order; at each i every lane walks ITS window -- from max(reach[c], i + 1), one element at a
//                       time, relaxing dist[e] with the strict `<` at every e it visits, until the edge reaches its budget or
//                       e == n -- exactly the host's inner loop, with the classes side by side instead of one after the other.
//                       Then one lane walks the parents back from n.
//   k_partition_gather  the end points of every item, compact, to their list's place in the side's output.
//
// Why the classes may walk side by side. On the host class c starts at max(reach[c], at_least), at_least being where class c - 1
// stopped at this i (or i + 1), and the forced advance to at_least skips budget checks. Write s_c = max(reach[c], i + 1) and f_c for
// where a walk with checks from s_c stops. reach is non-decreasing in c after every step (a class never ends before the cheaper
// one), so s_{c-1} <= s_c. If f_{c-1} > s_c, the walk of c - 1 passed every position of [s_c, f_{c-1}) with an edge below
// budget[c-1] < budget[c]: the walk of c from s_c passes them too, so f_c >= f_{c-1}, and a walk of c started AT f_{c-1} stops at
// the same f_c. Hence the host's class c ends at f_c whatever at_least was, and visits [max(s_c, f_{c-1}), f_c]; the positions
// [s_c, f_{c-1}) a lane visits in addition were visited by class c - 1 or, by the same argument, a cheaper one. An edge (i -> e) has
// one cost whoever visits it, and every relaxation of step i writes parent i: the SET of edges is the host's, and dist / parent
// after step i are the host's. Nothing here asks the cost to be monotone along a window; the walk is a walk, not a search.
// Lanes that meet at one e in one instruction store the same two values.
//
// dist (u64) and parent (u32) live per position in global scratch (12 bytes per posting and side): a consecutive run costs
// fix_cost at any length, so a window has no bound but n -- nothing assumes it fits a wavefront, LDS or a tile. Lanes of one
// wavefront exchange dist through memory: its vector memory operations are performed in program order (wavefront-scope atomics
// and fences cost no instruction, they only keep the compiler from holding a slot in a register across steps).
// Every loop is bounded by n: e only grows and stops at n; parent[p] < p for p > 0, so the walk back ends.
#include <hip/hip_runtime.h>

#include "device_codecs.hpp"
#include "launchers.hpp"
#include "seq_cost.hpp"

using namespace ds2i_dev;

namespace {

DS2I_DEV uint64_t slot_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
DS2I_DEV void slot_store(unsigned long long* p, uint64_t v) { __hip_atomic_store(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
DS2I_DEV uint32_t slot_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
DS2I_DEV void slot_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
DS2I_DEV void step_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

template <bool STRICT>
DS2I_DEV void plan_item(const PartArgs& a, const PartItem it, const uint32_t lane) {
    const ds2i_host::global_parameters params;
    const uint64_t in0 = a.list_in[it.list];
    const uint64_t n = a.list_in[it.list + 1] - in0; // >= 1 (checked on the host)
    auto value = [&](uint64_t p) -> uint64_t {
        if constexpr (STRICT) return a.cum[in0 + p];
        else return a.docs[in0 + p];
    };
    const uint64_t universe = STRICT ? value(n - 1) + 1 : a.num_docs;
    const uint64_t whole = ds2i_host::partition_cost<STRICT>(params, universe, n, a.fix_cost);
    unsigned long long* const dist = a.dist + it.base;
    uint32_t* const parent = a.parent + it.base;
    for (uint64_t p = lane; p <= n; p += 64) {
        slot_store(dist + p, p ? whole : 0);
        slot_store(parent + p, 0u);
    }
    // the classes of this sequence: the budgets up to the first that covers `whole` (optimal_partition breaks its list off there)
    const uint64_t my_budget = lane < a.nbudgets ? a.budget[lane] : ~uint64_t(0);
    const uint64_t covers = __ballot(lane < a.nbudgets && my_budget >= whole);
    const uint32_t nclasses = covers ? (uint32_t)__builtin_ctzll(covers) + 1u : a.nbudgets;
    const bool active = lane < nclasses;
    step_fence();

    uint64_t e = 0, top = 0; // this class's window end and the value before it (top == value(e - 1) once e > 0)
    uint64_t before = 0;     // value(i - 1)
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t vi = value(i);
        const uint64_t floor_value = i ? before + 1 : vi; // smallest value a partition starting at i can hold
        const uint64_t here = slot_load(dist + i);
        if (active) {
            if (e < i + 1) {
                e = i + 1;
                top = vi;
            }
            for (uint64_t left = n - i; left; --left) { // (e <= n grows by one a turn: at most n - i turns)
                const uint64_t known = slot_load(dist + e);
                const uint64_t next = e < n ? value(e) : 0;
                const uint64_t edge = ds2i_host::partition_cost<STRICT>(params, top - floor_value + 1, e - i, a.fix_cost);
                if (here + edge < known) {
                    slot_store(dist + e, here + edge);
                    slot_store(parent + e, (uint32_t)i);
                }
                if (e == n || edge >= my_budget) break;
                top = next;
                ++e;
            }
        }
        before = vi;
        step_fence();
    }
    // the parents back from n: partition k (counted from the last) ends at the k-th node of the chain. dist is done with, so the
    // end points go to the END of the item's dist slots (2 (n + 1) u32, at most n end points), last one first: they lie ascending
    uint32_t* const ends_top = (uint32_t*)(dist + n + 1);
    uint32_t count = 0;
    for (uint64_t p = n; p != 0 && count < n; p = slot_load(parent + p)) {
        ++count;
        if (lane == 0) *(ends_top - count) = (uint32_t)p;
    }
    if (lane == 0) a.count[it.side * a.nlists + it.list] = count;
}

__global__ void __launch_bounds__(64) k_partition_plan(PartArgs a) {
    const uint32_t lane = lane_id();
    const PartItem it = a.items[blockIdx.x];
    if (it.side) plan_item<true>(a, it, lane);
    else plan_item<false>(a, it, lane);
}

__global__ void __launch_bounds__(64) k_partition_gather(PartArgs a) {
    const uint32_t lane = lane_id();
    const PartItem it = a.items[blockIdx.x];
    const uint64_t n = a.list_in[it.list + 1] - a.list_in[it.list];
    const uint32_t count = a.count[it.side * a.nlists + it.list];
    if (count > n) return; // (never: the plan kernel counts at most n)
    const uint32_t* const src = (const uint32_t*)(a.dist + it.base + n + 1) - count;
    uint32_t* const dst = a.out_ends[it.side] + a.out_offs[it.side * (a.nlists + 1) + it.list];
    for (uint64_t k = lane; k < count; k += 64) dst[k] = src[k];
}

} // namespace

extern "C" hipError_t ds2i_launch_partition_plan(const PartArgs& a, hipStream_t s) {
    if (!a.nitems) return hipSuccess;
    if (a.nbudgets > PART_MAX_CLASSES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_partition_plan, dim3(a.nitems), dim3(64), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_partition_gather(const PartArgs& a, hipStream_t s) {
    if (!a.nitems) return hipSuccess;
    hipLaunchKernelGGL(k_partition_gather, dim3(a.nitems), dim3(64), 0, s, a);
    return hipGetLastError();
}
