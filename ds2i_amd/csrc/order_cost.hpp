// The integer arithmetic of ordering documents by recursive graph bisection, stated ONCE for the host twin (host_order.hpp) and the
// device (order_kernels.hip, capi_order.cpp): the segments of a level, the cost of moving one document's term across its segment, the
// clamp of a gain and the sort key of a clamped gain. Integers only; the same text is compiled for the host and for gfx950.
//
// Fixed point. LOGQ[x] = rint(log2(x) * 2^ORDER_FRAC_BITS) as u32 for 1 <= x <= num_docs + 2, LOGQ[0] = 0. The table is built on the
// host (host_order.hpp, order_log_table) and uploaded: no logarithm is evaluated on the device.
//
// Segments. Level l cuts the positions [0, num_docs) into 2^l segments; segment k is [order_bound(n, l, k), order_bound(n, l, k + 1)).
// Its halves are the level l + 1 segments 2k (left) and 2k + 1 (right).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DS2I_ORDER_HD __host__ __device__ inline
#else
#define DS2I_ORDER_HD inline
#endif

namespace ds2i_host {

constexpr uint32_t ORDER_FRAC_BITS = 8;
constexpr uint32_t ORDER_DEFAULT_ITERATIONS = 20, ORDER_DEFAULT_MIN_HALF = 16, ORDER_DEFAULT_MAX_LEVELS = 32;
constexpr uint32_t ORDER_MAX_ITERATIONS = 1u << 16, ORDER_MAX_LEVELS = 32;
constexpr uint64_t ORDER_MAX_DOCS = 0xFFFFFFFEull; // num_docs must stay below it: LOGQ is indexed up to num_docs + 2 in 32 bits

// b_l(k) = (k * n) >> l; k <= 2^l <= 2^32 and n < 2^32, so the product fits 64 bits
DS2I_ORDER_HD uint64_t order_bound(uint64_t n, uint32_t level, uint64_t k) { return (k * n) >> level; }

// the level `level` segment that holds position p (< n): the largest k with b(k) <= p. b(k) <= p <=> k * n < (p + 1) << level, and
// (p + 1) << level < 2^64 for p + 1 < 2^32 and level <= 32.
DS2I_ORDER_HD uint32_t order_segment_of(uint64_t n, uint32_t level, uint64_t p) { return (uint32_t)((((p + 1) << level) - 1) / n); }

// What one term contributes to the gain of moving a document from its side (size na, the term's degree there da >= 1, the document
// included) to the other (size nb, degree db): the cost of the term's two degrees now, minus the cost after the move. Every product is
// below 2^32 * 2^13; the arithmetic wraps in 64 bits like the sums it goes into.
DS2I_ORDER_HD int64_t order_term_cost(const uint32_t* logq, uint32_t na, uint32_t nb, uint32_t da, uint32_t db) {
    const int64_t la = logq[na], lb = logq[nb];
    const int64_t c = (int64_t)da * (la - (int64_t)logq[da + 1]) + (int64_t)db * (lb - (int64_t)logq[db + 1]) -
                      (int64_t)(da - 1) * (la - (int64_t)logq[da]) - (int64_t)(db + 1) * (lb - (int64_t)logq[db + 2]);
    return c;
}

// a document's gain as the sort and the swap see it
DS2I_ORDER_HD int32_t order_clamp_gain(int64_t g) {
    return g > (int64_t)INT32_MAX ? INT32_MAX : g < (int64_t)INT32_MIN ? INT32_MIN : (int32_t)g;
}
// the order-reversing u32 image of a clamped gain: a larger gain has a smaller key, so an ascending sort gives gains descending
DS2I_ORDER_HD uint32_t order_gain_key(int32_t g) { return ~((uint32_t)g ^ 0x80000000u); }
DS2I_ORDER_HD int32_t order_key_gain(uint32_t key) { return (int32_t)(~key ^ 0x80000000u); }

} // namespace ds2i_host
