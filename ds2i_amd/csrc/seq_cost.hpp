// The closed forms of the Elias-Fano family's sizes, stated ONCE for the host builder (host_index.hpp, host_pef.hpp), the host
// planner (host_freq_plan.hpp) and the device partition planner (partition_kernels.hip): every size of these layouts is an integer
// function of (universe, n) and the sampling parameters.
//   global_parameters        reference global_parameters.hpp:5-31
//   ef_offsets               reference compact_elias_fano.hpp:14-61
//   rb_offsets               reference compact_ranked_bitvector.hpp:14-45
//   seq_bitsize              reference indexed_sequence.hpp:23-60, strict_sequence.hpp:24-60
//   partition_cost           the edge cost of optimal_partition (partitioned_sequence.hpp:35-41: bitsize + fix_cost)
// Integers only (one 64-bit division); the same text is compiled for the host and for gfx950.
#pragma once
#include <cassert>
#include <cstdint>

#if defined(__HIPCC__)
#define DS2I_HD __host__ __device__ inline
#else
#define DS2I_HD inline
#endif

namespace ds2i_host {

DS2I_HD uint32_t msb64(uint64_t x) {
#if !defined(__HIP_DEVICE_COMPILE__)
    assert(x);
#endif
    return 63u - (uint32_t)__builtin_clzll(x);
}
// util.hpp:30-33
DS2I_HD uint64_t ceil_log2(uint64_t x) { return x > 1 ? msb64(x - 1) + 1 : 0; }

struct global_parameters {
    uint8_t ef_log_sampling0 = 9, ef_log_sampling1 = 8, rb_log_rank1_sampling = 9, rb_log_sampling1 = 8,
            log_partition_size = 7;
};

// ------------------------------------------------------------ Elias-Fano (a13)
struct ef_offsets {
    uint64_t universe, n, log_sampling0, log_sampling1, lower_bits, mask, higher_bits_length, pointer_size,
        pointers0, pointers1, pointers0_offset, pointers1_offset, higher_bits_offset, lower_bits_offset, end;
    DS2I_HD ef_offsets(uint64_t base, uint64_t u, uint64_t n_, global_parameters const& p)
        : universe(u), n(n_), log_sampling0(p.ef_log_sampling0), log_sampling1(p.ef_log_sampling1) {
        lower_bits = u > n ? msb64(u / n) : 0;
        mask = (uint64_t(1) << lower_bits) - 1;
        higher_bits_length = n + (u >> lower_bits) + 2;
        pointer_size = ceil_log2(higher_bits_length);
        pointers0 = (higher_bits_length - n) >> log_sampling0;
        pointers1 = n >> log_sampling1;
        pointers0_offset = base;
        pointers1_offset = pointers0_offset + pointers0 * pointer_size;
        higher_bits_offset = pointers1_offset + pointers1 * pointer_size;
        lower_bits_offset = higher_bits_offset + higher_bits_length;
        end = lower_bits_offset + n * lower_bits;
    }
};

// ------------------------------------------------------------ ranked bitvector
struct rb_offsets {
    uint64_t universe, n, log_rank1_sampling, log_sampling1, rank1_sample_size, pointer_size, rank1_samples, pointers1,
        rank1_samples_offset, pointers1_offset, bits_offset, end;
    DS2I_HD rb_offsets(uint64_t base, uint64_t u, uint64_t n_, global_parameters const& p)
        : universe(u), n(n_), log_rank1_sampling(p.rb_log_rank1_sampling), log_sampling1(p.rb_log_sampling1) {
        rank1_sample_size = ceil_log2(n + 1);
        pointer_size = ceil_log2(u);
        rank1_samples = log_rank1_sampling >= 64 ? 0 : (u >> log_rank1_sampling);
        pointers1 = n >> log_sampling1;
        rank1_samples_offset = base;
        pointers1_offset = rank1_samples_offset + rank1_samples * rank1_sample_size;
        bits_offset = pointers1_offset + pointers1 * pointer_size;
        end = bits_offset + u;
    }
};
DS2I_HD uint64_t rb_bitsize(global_parameters const& p, uint64_t u, uint64_t n) { return rb_offsets(0, u, n, p).end; }
DS2I_HD uint64_t ef_bitsize(global_parameters const& p, uint64_t u, uint64_t n) { return ef_offsets(0, u, n, p).end; }

// ------------------------------------------------------------ indexed / strict sequences
enum seq_type : int { SEQ_EF = 0, SEQ_RB = 1, SEQ_ALL_ONES = 2 };
constexpr uint64_t SEQ_TYPE_BITS = 1;

DS2I_HD global_parameters strict_params(global_parameters p) {
    p.ef_log_sampling0 = 63;
    p.rb_log_rank1_sampling = 63;
    return p;
}

template <bool STRICT>
DS2I_HD uint64_t seq_bitsize(global_parameters const& params, uint64_t universe, uint64_t n, int* type_out = nullptr) {
    uint64_t best = (universe == n) ? 0 : uint64_t(-1);
    int type = SEQ_ALL_ONES;
    if (best) {
        const global_parameters sp = STRICT ? strict_params(params) : params;
        uint64_t ef = (STRICT ? ef_bitsize(sp, universe - n + 1, n) : ef_bitsize(sp, universe, n)) + SEQ_TYPE_BITS;
        if (ef < best) { best = ef; type = SEQ_EF; }
        uint64_t rb = rb_bitsize(sp, universe, n) + SEQ_TYPE_BITS;
        if (rb < best) { best = rb; type = SEQ_RB; }
    }
    if (type_out) *type_out = type;
    return best;
}

// what one partition of m elements spanning u values costs the partition DP
template <bool STRICT>
DS2I_HD uint64_t partition_cost(global_parameters const& params, uint64_t u, uint64_t m, uint64_t fix_cost) {
    return seq_bitsize<STRICT>(params, u, m) + fix_cost;
}

} // namespace ds2i_host
