// HIP kernels (gfx950, wave64) that WRITE the Elias-Fano layouts -- opt, ef, single, uniform (index_types.hpp:18-32): the build-side
// counterpart of device_pef.hpp. The host plans (host_freq_plan.hpp): every size of these layouts is a closed form of (universe, n),
// so it knows the type, the length and the final bit offset of every base sequence without looking at the values, and writes the
// headers itself. The device writes the bodies -- everything seq_write / ef_write / rb_write (host_pef.hpp, host_index.hpp) emit:
//   k_freq_block_sums / k_freq_list_scan / k_freq_prefix   the 64-bit prefix sums of every list's freqs (positive_sequence), over the
//                     block tables of the CSR staging: per-block sums, a scan of every list's block sums, the scan inside a block
//   k_freq_write      one THREAD per posting and side. It finds its base sequence (FreqJob, abi_structs.hpp) by binary search over
//                     the jobs' first postings and ORs its own bits into the zero-filled bit vector:
//                       Elias-Fano        high bit (v >> l) + i + 1, low field at i * l
//                       ranked bitvector  bit v of the characteristic vector
//                     and the sampled entries that follow from ITS element alone, from what they mean (the second pass of ef_write
//                     / rb_write): pointers1[k - 1] is the position of element k * 2^s1; the zeros (EF) / the sampled positions (RB)
//                     between the previous element and this one all have i ones before them, so the pointers0 / rank1_samples
//                     entries that fall there are this element's; the last element also owns what follows it.
// Nothing assumes that a base sequence fits a wavefront or LDS: a one-element partition and a list of 25 M postings take the same
// path. Neighbouring sequences and the host's headers share words, so every write is a 64-bit atomicOr into the zeroed vector (a
// field that straddles a word: two). OR does not depend on order: the result is the host's, bit for bit, at any grid.
#include <hip/hip_runtime.h>

#include "device_codecs.hpp"
#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

constexpr uint32_t FQ_WAVES = 4;    // prefix-sum kernels: waves per workgroup, a 128-posting block (or a list) each
constexpr uint32_t FQ_THREADS = 256; // k_freq_write

struct PrefixArgs {
    const uint32_t* freqs;
    const uint64_t* list_in;   // nlists + 1 posting offsets
    const uint32_t* blk_list;  // per block: its list
    const uint32_t* list_blk0; // per list: its first block (global numbering)
    uint32_t nblocks;
    uint64_t nlists;
    unsigned long long* blk_base; // per block: its sum, then (k_freq_list_scan) the sum of the list's blocks before it
    unsigned long long* cum;      // per posting: inclusive prefix sum of its list's freqs
};

DS2I_DEV uint64_t bcast64(uint64_t v, uint32_t src) { return ((uint64_t)bcast((uint32_t)(v >> 32), src) << 32) | bcast((uint32_t)v, src); }

// inclusive wave scan of 32-bit values as 64-bit sums: the two 16-bit halves scan separately (64 * 65535 < 2^32)
DS2I_DEV uint64_t wave_incl_scan_wide(uint32_t x) {
    const uint32_t lo = wave_incl_scan(x & 0xFFFFu), hi = wave_incl_scan(x >> 16);
    return ((uint64_t)hi << 16) + lo;
}
// ... of 64-bit values (sums that stay below 2^64: a list's occurrences): four 16-bit pieces
DS2I_DEV uint64_t wave_incl_scan64(uint64_t x) {
    const uint64_t lo = wave_incl_scan_wide((uint32_t)x), hi = wave_incl_scan_wide((uint32_t)(x >> 32));
    return (hi << 32) + lo;
}

struct BlockOfList {
    uint64_t k0; // first posting
    uint32_t sz;
};
DS2I_DEV BlockOfList block_of(const PrefixArgs& a, uint64_t blk) {
    const uint32_t t = a.blk_list[blk];
    const uint32_t lb = (uint32_t)blk - a.list_blk0[t];
    const uint64_t in0 = a.list_in[t];
    const uint64_t left = a.list_in[t + 1] - in0 - 128ull * lb;
    return {in0 + 128ull * lb, left < 128u ? (uint32_t)left : 128u};
}

__global__ void __launch_bounds__(64 * FQ_WAVES) k_freq_block_sums(PrefixArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    for (uint64_t blk = (uint64_t)blockIdx.x * FQ_WAVES + wave; blk < a.nblocks; blk += (uint64_t)gridDim.x * FQ_WAVES) {
        const BlockOfList b = block_of(a, blk);
        const uint32_t v0 = lane < b.sz ? a.freqs[b.k0 + lane] : 0u;
        const uint32_t v1 = lane + 64u < b.sz ? a.freqs[b.k0 + 64u + lane] : 0u;
        const uint64_t sum = wave_incl_scan_wide(v0) + wave_incl_scan_wide(v1);
        if (lane == 63) a.blk_base[blk] = sum;
    }
}

// one wavefront per list: exclusive scan of its blocks' sums, 64 blocks a step
__global__ void __launch_bounds__(64 * FQ_WAVES) k_freq_list_scan(PrefixArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    for (uint64_t t = (uint64_t)blockIdx.x * FQ_WAVES + wave; t < a.nlists; t += (uint64_t)gridDim.x * FQ_WAVES) {
        const uint64_t nb = (a.list_in[t + 1] - a.list_in[t] + 127u) / 128u;
        unsigned long long* const base = a.blk_base + a.list_blk0[t];
        uint64_t carry = 0;
        for (uint64_t c = 0; c < nb; c += 64) {
            const uint64_t x = c + lane < nb ? base[c + lane] : 0;
            const uint64_t incl = wave_incl_scan64(x);
            if (c + lane < nb) base[c + lane] = carry + incl - x;
            carry += bcast64(incl, 63);
        }
    }
}

__global__ void __launch_bounds__(64 * FQ_WAVES) k_freq_prefix(PrefixArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x >> 6);
    for (uint64_t blk = (uint64_t)blockIdx.x * FQ_WAVES + wave; blk < a.nblocks; blk += (uint64_t)gridDim.x * FQ_WAVES) {
        const BlockOfList b = block_of(a, blk);
        const uint32_t v0 = lane < b.sz ? a.freqs[b.k0 + lane] : 0u;
        const uint32_t v1 = lane + 64u < b.sz ? a.freqs[b.k0 + 64u + lane] : 0u;
        const uint64_t before = a.blk_base[blk];
        const uint64_t s0 = wave_incl_scan_wide(v0);
        const uint64_t s1 = wave_incl_scan_wide(v1) + bcast64(s0, 63);
        if (lane < b.sz) a.cum[b.k0 + lane] = before + s0;
        if (lane + 64u < b.sz) a.cum[b.k0 + 64u + lane] = before + s1;
    }
}

// ---------------------------------------------------------------- the bodies
// len (<= 64) bits of v (< 2^len) at bit `pos`. A field that would end past the vector is a layout error and is dropped: the
// kernel never writes outside [0, nbits) (the buffer holds two more words than that)
DS2I_DEV void or_field(const FreqEncArgs& a, uint64_t pos, uint64_t v, uint32_t len) {
    if (!len || pos + len > a.nbits) return;
    const uint32_t sh = (uint32_t)(pos & 63u);
    const uint64_t w = pos >> 6;
    const uint64_t lo = v << sh;
    if (lo) atomicOr(a.out + w, (unsigned long long)lo);
    if (sh + len > 64u) {
        const uint64_t hi = v >> (64u - sh);
        if (hi) atomicOr(a.out + w + 1, (unsigned long long)hi);
    }
}

// the entries k (>= 1) of a sampled array whose sampled quantity k << ls lies in [from, to]: entry k - 1 = (k << ls) + add (EF
// pointers0: the position of that zero) or `add` alone (RB rank1_samples: the ones before that position)
template <bool POSITION>
DS2I_DEV void or_samples(const FreqEncArgs& a, const FreqJob& J, uint64_t from, uint64_t to, uint64_t add) {
    const uint64_t step = uint64_t(1) << J.lsa;
    uint64_t k = (from + step - 1) >> J.lsa;
    if (!k) k = 1;
    for (; k <= J.na && (k << J.lsa) <= to; ++k) or_field(a, J.a_off + (k - 1) * J.wa, POSITION ? (k << J.lsa) + add : add, J.wa);
}

template <bool FREQS>
__global__ void __launch_bounds__(FQ_THREADS) k_freq_write(FreqEncArgs a) {
    for (uint64_t k = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x; k < a.postings; k += (uint64_t)gridDim.x * FQ_THREADS) {
        uint64_t j = 0, above = a.njobs; // the last job with src <= k (jobs[0].src == 0)
        while (above - j > 1) {
            const uint64_t mid = (j + above) >> 1;
            if (a.jobs[mid].src <= k) j = mid;
            else above = mid;
        }
        const FreqJob J = a.jobs[j];
        const uint64_t i = k - J.src;
        if (i >= J.n || J.type == FREQ_SEQ_ALL_ONES) continue;
        auto value = [&](uint64_t p) -> uint64_t {
            if constexpr (FREQS) return a.cum[p];
            else return a.docs[p];
        };
        const uint64_t v = value(k) - J.origin - (J.shift ? i : 0);
        const uint64_t vp = i ? value(k - 1) - J.origin - (J.shift ? i - 1 : 0) : 0; // the element before, stored the same way
        const bool last = i + 1 == J.n;
        const bool sampled1 = J.nb && i && !(i & ((uint64_t(1) << J.lsb) - 1)) && (i >> J.lsb) <= J.nb;
        if (J.type == FREQ_SEQ_EF) {
            const uint64_t h = v >> J.l, pos = h + i + 1;
            or_field(a, J.hi_off + pos, 1, 1);
            if (J.l) or_field(a, J.lo_off + i * J.l, v & ((uint64_t(1) << J.l) - 1), J.l);
            if (sampled1) or_field(a, J.b_off + ((i >> J.lsb) - 1) * J.wb, pos, J.wb);
            if (J.na) { // zero number z sits at z + (ones before it); the zeros (h of i - 1, h] have i ones before them
                or_samples<true>(a, J, i ? (vp >> J.l) + 1 : 0, h, i);
                if (last) or_samples<true>(a, J, h + 1, J.hi_len - J.n - 1, J.n);
            }
        } else {
            if (!i && J.typed) or_field(a, J.type_off, FREQ_SEQ_RB, 1);
            or_field(a, J.hi_off + v, 1, 1);
            if (sampled1) or_field(a, J.b_off + ((i >> J.lsb) - 1) * J.wb, v, J.wb);
            if (J.na) { // the positions (v of i - 1, v] have i ones before them
                or_samples<false>(a, J, i ? vp + 1 : 0, v, i);
                if (last && v + 1 < J.hi_len) or_samples<false>(a, J, v + 1, J.hi_len - 1, J.n);
            }
        }
    }
}

unsigned grid_for(uint64_t items, uint64_t per_group, unsigned max_groups) {
    uint64_t g = (items + per_group - 1) / per_group;
    if (g > max_groups) g = max_groups;
    return g ? (unsigned)g : 1u;
}

} // namespace

extern "C" hipError_t ds2i_launch_freq_prefix_sums(const EncArgs& st, uint64_t nlists, uint64_t* blk_base, uint64_t* cum, unsigned max_groups,
                                                   hipStream_t s) {
    PrefixArgs a;
    a.freqs = st.freqs;
    a.list_in = st.list_in;
    a.blk_list = st.blk_list;
    a.list_blk0 = st.list_blk0;
    a.nblocks = st.nblocks;
    a.nlists = nlists;
    a.blk_base = (unsigned long long*)blk_base;
    a.cum = (unsigned long long*)cum;
    const unsigned per_block = grid_for(st.nblocks, FQ_WAVES, max_groups);
    hipLaunchKernelGGL(k_freq_block_sums, dim3(per_block), dim3(64 * FQ_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_freq_list_scan, dim3(grid_for(nlists, FQ_WAVES, max_groups)), dim3(64 * FQ_WAVES), 0, s, a);
    hipLaunchKernelGGL(k_freq_prefix, dim3(per_block), dim3(64 * FQ_WAVES), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t ds2i_launch_freq_write(int freqs_side, const FreqEncArgs& a, unsigned max_groups, hipStream_t s) {
    if (!a.njobs || !a.postings) return hipSuccess;
    const unsigned grid = grid_for(a.postings, FQ_THREADS, max_groups);
    if (freqs_side) hipLaunchKernelGGL(k_freq_write<true>, dim3(grid), dim3(FQ_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_freq_write<false>, dim3(grid), dim3(FQ_THREADS), 0, s, a);
    return hipGetLastError();
}
