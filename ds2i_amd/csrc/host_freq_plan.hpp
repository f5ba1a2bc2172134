// Host half of the GPU encoder of the Elias-Fano layouts (opt, ef, single, uniform; capi_encode.cpp, freq_encode_kernels.hip).
// The sequence writers of host_pef.hpp run here unchanged, with a `Bodies` that does not encode: for every base sequence it takes
// (universe, n) -- seq_bitsize / ef_offsets / rb_offsets give its type, its exact length and the place of each of its arrays
// without looking at the values -- and records a FreqJob for the device. What the writers put into the bit builder is then the
// list's HEADER alone (gamma / delta codes, first value, the EF of the bounds and inner ends, the end offsets), which always
// precedes the list's base sequences. A list side = header | base sequences back to back.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "abi_structs.hpp"
#include "host_parallel.hpp"
#include "host_pef.hpp"

namespace ds2i_host {

// Sizes the base sequences of one side of one list; offsets are relative to the first of them until `place` moves them.
template <bool STRICT>
struct planned_bodies {
    const uint64_t* seq = nullptr;
    global_parameters params;
    uint64_t src = 0;   // global index of the list's first posting
    uint64_t bits = 0;
    std::vector<ds2i_dev::FreqJob>& jobs;
    planned_bodies(global_parameters const& p, uint64_t first_posting, std::vector<ds2i_dev::FreqJob>& out)
        : params(p), src(first_posting), jobs(out) {}
    uint64_t size() const { return bits; }

    void partition(uint64_t from, uint64_t to, uint64_t origin) { typed(from, to - from, origin, seq[to - 1] - origin + 1); }
    void whole(uint64_t universe, uint64_t n) { typed(0, n, 0, universe); }
    void whole_ef(uint64_t universe, uint64_t n) { // the index's own parameters, no type bit
        ds2i_dev::FreqJob j = job(0, n, 0);
        elias_fano(j, ef_offsets(bits, STRICT ? universe - n + 1 : universe, n, params));
        push(j, ef_bitsize(params, STRICT ? universe - n + 1 : universe, n));
    }
    void append_to(bitvec_builder const&) {}

private:
    ds2i_dev::FreqJob job(uint64_t from, uint64_t n, uint64_t origin) const {
        ds2i_dev::FreqJob j{};
        j.src = src + from;
        j.n = n;
        j.origin = origin;
        j.type_off = bits;
        return j;
    }
    static void elias_fano(ds2i_dev::FreqJob& j, ef_offsets const& of) {
        j.type = ds2i_dev::FREQ_SEQ_EF;
        j.shift = STRICT;
        j.a_off = of.pointers0_offset;
        j.b_off = of.pointers1_offset;
        j.hi_off = of.higher_bits_offset;
        j.lo_off = of.lower_bits_offset;
        j.hi_len = of.higher_bits_length;
        j.na = of.pointers0;
        j.nb = of.pointers1;
        j.l = (uint8_t)of.lower_bits;
        j.wa = j.wb = (uint8_t)of.pointer_size;
        j.lsa = (uint8_t)of.log_sampling0;
        j.lsb = (uint8_t)of.log_sampling1;
    }
    void push(ds2i_dev::FreqJob const& j, uint64_t cost) {
        jobs.push_back(j);
        bits += cost;
    }
    // seq_write<STRICT>: the type bit, then the cheapest of Elias-Fano, ranked bitvector and nothing (all ones)
    void typed(uint64_t from, uint64_t n, uint64_t origin, uint64_t universe) {
        int type;
        const uint64_t cost = seq_bitsize<STRICT>(params, universe, n, &type);
        const global_parameters sp = STRICT ? strict_params(params) : params;
        ds2i_dev::FreqJob j = job(from, n, origin);
        j.typed = 1;
        j.type = ds2i_dev::FREQ_SEQ_ALL_ONES;
        if (type == SEQ_EF) {
            elias_fano(j, ef_offsets(bits + SEQ_TYPE_BITS, STRICT ? universe - n + 1 : universe, n, sp));
        } else if (type == SEQ_RB) {
            const rb_offsets of(bits + SEQ_TYPE_BITS, universe, n, sp);
            j.type = ds2i_dev::FREQ_SEQ_RB;
            j.a_off = of.rank1_samples_offset;
            j.b_off = of.pointers1_offset;
            j.hi_off = of.bits_offset;
            j.hi_len = universe;
            j.na = of.rank1_samples;
            j.nb = of.pointers1;
            j.wa = (uint8_t)of.rank1_sample_size;
            j.wb = (uint8_t)of.pointer_size;
            j.lsa = (uint8_t)of.log_rank1_sampling;
            j.lsb = (uint8_t)of.log_sampling1;
        }
        push(j, cost);
    }
};
static_assert((int)ds2i_dev::FREQ_SEQ_EF == SEQ_EF && (int)ds2i_dev::FREQ_SEQ_RB == SEQ_RB && (int)ds2i_dev::FREQ_SEQ_ALL_ONES == SEQ_ALL_ONES,
              "the device's sequence types are seq_type");

// moves a job by `delta` bits
inline void place(ds2i_dev::FreqJob& j, uint64_t delta) {
    j.type_off += delta;
    j.a_off += delta;
    j.b_off += delta;
    j.hi_off += delta;
    j.lo_off += delta;
}

// One list as the device encoder sees it. side 0 = docs, 1 = freqs.
struct freq_list_plan {
    bitvec_builder head[2];                  // the headers, as the host builder writes them
    uint64_t body_bits[2] = {0, 0};          // bits of the base sequences that follow the header
    std::vector<ds2i_dev::FreqJob> jobs[2];  // offsets relative to the end of the header
};

// opt_index_builder::encode_list with the base sequences planned instead of written. For opt this runs optimal_partition, unless
// the end points of the two sides are given (docs_ends, freqs_ends: the device planner's)
inline void plan_list(int layout, uint64_t num_docs, global_parameters const& params, uint64_t first_posting, uint64_t n,
                      const uint32_t* docs, const uint32_t* freqs, freq_list_plan& out, const std::vector<uint32_t>* docs_ends = nullptr,
                      const std::vector<uint32_t>* freqs_ends = nullptr) {
    planned_bodies<false> db(params, first_posting, out.jobs[0]);
    planned_bodies<true> fb(params, first_posting, out.jobs[1]);
    opt_index_builder::encode_list(num_docs, params, n, docs, freqs, out.head[0], out.head[1], layout, db, fb, docs_ends, freqs_ends);
    out.body_bits[0] = db.size();
    out.body_bits[1] = fb.size();
}

// What the Elias-Fano layouts rely on: no empty list, doc-ids strictly increasing and below num_docs (the sequences are sorted sets
// over that universe), every freq >= 1 (a zero makes the prefix sums non-strict). Empty, or the message of the first violation.
inline std::string freq_postings_fault(const char* who, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs,
                                       const uint32_t* freqs) {
    const std::string w(who);
    for (uint64_t t = 0; t < nlists; ++t) {
        if (offs[t + 1] <= offs[t]) return "List must be nonempty";
        if (offs[t + 1] - offs[t] > 0xFFFFFFFFull) return "posting list longer than 2^32";
        for (uint64_t i = offs[t]; i < offs[t + 1]; ++i) {
            if (i > offs[t] && docs[i] <= docs[i - 1]) return w + ": doc ids not strictly increasing";
            if (docs[i] >= num_docs) return w + ": doc id out of range";
            if (!freqs[i]) return w + ": zero freq";
        }
    }
    return std::string();
}

// The partition end points of the opt layout for every list of a CSR collection: ends[side] holds every list's end points back to
// back, offs[side][t] .. offs[side][t + 1] those of list t (side 0 = docs over num_docs, 1 = the prefix sums over occurrences + 1)
struct opt_partitions {
    std::vector<uint32_t> ends[2];
    std::vector<uint64_t> offs[2];
    std::vector<uint32_t> of(int side, uint64_t t) const {
        return std::vector<uint32_t>(ends[side].begin() + offs[side][t], ends[side].begin() + offs[side][t + 1]);
    }
};
// ... of one list, planned on the host (what partitioned_write plans for the two sides of encode_list)
inline void host_list_partitions(uint64_t num_docs, global_parameters const& params, uint64_t n, const uint32_t* docs,
                                 const uint32_t* freqs, std::vector<uint32_t> ends[2]) {
    std::vector<uint64_t> d(n), cum(n);
    uint64_t occurrences = 0;
    for (uint64_t i = 0; i < n; ++i) {
        d[i] = docs[i];
        occurrences += freqs[i];
        cum[i] = occurrences;
    }
    ends[0] = partition_ends<false>(d.data(), num_docs, n, params);
    ends[1] = partition_ends<true>(cum.data(), occurrences + 1, n, params);
}

// the planning pool: the calling thread and up to FREQ_PLAN_THREADS - 1 more -- never the whole machine's CPU count, never more
// threads than lists
constexpr unsigned FREQ_PLAN_THREADS = 16;
inline unsigned plan_threads(uint64_t nlists) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (unsigned)std::min<uint64_t>(std::min(hw, FREQ_PLAN_THREADS), std::max<uint64_t>(nlists, 1));
}
// ... of every list of a collection, list-parallel: the reference of the device planner
inline void host_opt_partitions(uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs, const uint32_t* freqs,
                                opt_partitions& out) {
    const global_parameters params;
    std::vector<std::vector<uint32_t>> ends[2];
    ends[0].resize(nlists);
    ends[1].resize(nlists);
    parallel_for(nlists, plan_threads(nlists), [&](uint64_t t, unsigned) {
        std::vector<uint32_t> e[2];
        host_list_partitions(num_docs, params, offs[t + 1] - offs[t], docs + offs[t], freqs + offs[t], e);
        ends[0][t] = std::move(e[0]);
        ends[1][t] = std::move(e[1]);
    }, true);
    for (int side = 0; side < 2; ++side) {
        out.ends[side].clear();
        out.offs[side].assign(nlists + 1, 0);
        for (uint64_t t = 0; t < nlists; ++t) {
            out.ends[side].insert(out.ends[side].end(), ends[side][t].begin(), ends[side][t].end());
            out.offs[side][t + 1] = out.ends[side].size();
        }
    }
}

// ORs the `n` bits of `src` into `dst` at bit `pos`, touching only the words they cover
inline void or_bits_at(std::vector<uint64_t>& dst, uint64_t pos, bitvec_builder const& src) {
    const uint64_t n = src.size();
    auto const& w = src.words();
    const unsigned sh = (unsigned)(pos & 63);
    for (uint64_t i = 0, at = pos >> 6; i < n; i += 64, ++at) {
        const uint64_t bits = w[i >> 6];
        dst[at] |= bits << sh;
        if (sh && (bits >> (64 - sh))) dst[at + 1] |= bits >> (64 - sh);
    }
}

} // namespace ds2i_host
