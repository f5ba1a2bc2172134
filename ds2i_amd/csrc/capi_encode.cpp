// Host side of the GPU index encoder (include/ds2i_hip.h: ds2i_hip_encode_index): uploads the
// postings, runs the plan pass (findBestB per block part, sizes), lays the lists out from the sizes
// (block_posting_list::write's layout, block_posting_list.hpp:13-53), runs the write pass, and freezes the
// block_freq_index image around the device-written list bytes (block_freq_index.hpp:18-70, 124-134).
// The block_mixed optimiser's device half lives here too (ds2i_hip_hybrid_analyse / ds2i_hip_hybrid_freeze; §8(f) item
// 3): the plan kernel measures every candidate of every part, the host builds hulls and solves the budget
// (host_hybrid.hpp, shared with the host path), and one write pass lays the chosen encodings down.
// The wand_data image is built over the same staging (ds2i_hip_build_wand; ds2i_hip_build_collection returns it together
// with the index image from ONE upload): norm_lens on the host as compute_norm_lens writes them, every list's maximum
// term weight by wand_kernels.hip.
// The Elias-Fano layouts (opt, ef, single, uniform) go through the same entry points and the same staging: the host plans every
// list (host_freq_plan.hpp: headers, and the place of every base sequence), freq_encode_kernels.hip writes the base sequences.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/ds2i_build.h"
#include "capi_blob.hpp"
#include "capi_hybrid.hpp"
#include "capi_partition.hpp"
#include "capi_util.hpp"
#include "host_freq_plan.hpp"
#include "host_index.hpp"
#include "host_parallel.hpp"
#include "host_synth.hpp"
#include "launchers.hpp"

namespace {
#define STAGE_OK(call)                 \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != DS2I_OK) return rc_; \
    } while (0)

// A collection in CSR form staged on the device, with the block tables both kernels walk
struct EncStage {
    DevTemps dev;
    ds2i_dev::EncArgs a{};
    uint64_t nlists = 0, nblocks = 0;
    const uint64_t* list_offsets = nullptr;
    std::vector<uint32_t> list_blk0;
    unsigned grid = 1;
    uint64_t* d_blk_out = nullptr;
    uint64_t* d_list_out = nullptr;

    // the two ways in: upload() copies the postings from the host, adopt() takes postings that are on the device already (the
    // extraction kernels' output: a conversion never sends them over the bus again) and frees them with the staging
    int upload(const char* who, int device, uint64_t nl, const uint64_t* offs, const uint32_t* docs, const uint32_t* freqs) {
        STAGE_OK(tables(who, device, nl, offs));
        const uint64_t total = offs[nlists];
        uint32_t *d_docs, *d_freqs;
        HIP_OK(dev.alloc(&d_docs, 4 * total));
        HIP_OK(dev.alloc(&d_freqs, 4 * total));
        HIP_OK(hipMemcpy(d_docs, docs, 4 * total, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_freqs, freqs, 4 * total, hipMemcpyHostToDevice));
        a.docs = d_docs;
        a.freqs = d_freqs;
        return DS2I_OK;
    }
    int adopt(const char* who, int device, uint64_t nl, const uint64_t* offs, uint32_t* d_docs, uint32_t* d_freqs) {
        dev.p.push_back(d_docs); // (owned from here on, whatever happens below)
        dev.p.push_back(d_freqs);
        a.docs = d_docs;
        a.freqs = d_freqs;
        return tables(who, device, nl, offs);
    }

    // everything of the staging but the postings: the offsets and the block tables
    int tables(const char* who, int device, uint64_t nl, const uint64_t* offs) {
        const int rc = check_device(who, device);
        if (rc != DS2I_OK) return rc;
        nlists = nl;
        list_offsets = offs;
        std::vector<uint32_t> blk_list;
        list_blk0.resize(nlists);
        for (uint64_t t = 0; t < nlists; ++t) {
            if (offs[t + 1] <= offs[t]) return ds2i_set_error(DS2I_EINVAL, "List must be nonempty"); // block_freq_index.hpp:31
            const uint64_t n = offs[t + 1] - offs[t];
            if (n > 0xFFFFFFFFull) return ds2i_set_error(DS2I_EINVAL, "posting list longer than 2^32");
            list_blk0[t] = (uint32_t)nblocks;
            nblocks += (n + 127) / 128;
        }
        if (nblocks >= (1ull << 32)) return ds2i_set_error(DS2I_EINVAL, "more than 2^32 blocks");
        DS2I_TRY
        blk_list.resize(nblocks);
        DS2I_CATCH
        for (uint64_t t = 0; t < nlists; ++t) {
            const uint64_t nb = (offs[t + 1] - offs[t] + 127) / 128;
            std::fill(blk_list.begin() + list_blk0[t], blk_list.begin() + list_blk0[t] + nb, (uint32_t)t);
        }
        HIP_OK(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_OK(hipGetDeviceProperties(&prop, device));
        grid = (unsigned)std::min<uint64_t>(nblocks ? nblocks : 1, (uint64_t)(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256) * 32);
        uint32_t *d_blk_list, *d_list_blk0;
        uint64_t* d_list_in;
        HIP_OK(dev.alloc(&d_list_in, 8 * (nlists + 1)));
        HIP_OK(dev.alloc(&d_blk_list, 4 * nblocks));
        HIP_OK(dev.alloc(&d_list_blk0, 4 * nlists));
        HIP_OK(dev.alloc(&a.bsel, 2 * nblocks));
        HIP_OK(dev.alloc(&a.psize, 8 * nblocks));
        HIP_OK(dev.alloc(&a.bmax, 4 * nblocks));
        HIP_OK(dev.alloc(&d_blk_out, 8 * (nblocks + 1)));
        HIP_OK(dev.alloc(&d_list_out, 8 * nlists));
        HIP_OK(hipMemcpy(d_list_in, offs, 8 * (nlists + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_blk_list, blk_list.data(), 4 * nblocks, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_list_blk0, list_blk0.data(), 4 * nlists, hipMemcpyHostToDevice));
        a.list_in = d_list_in;
        a.blk_list = d_blk_list;
        a.list_blk0 = d_list_blk0;
        a.nblocks = (uint32_t)nblocks;
        return DS2I_OK;
    }

    // layout from the part sizes (2 per block): vbyte(n) | block_max[nb] | block_endpoint[nb - 1] | blocks (docs part,
    // freqs part each); allocates the output and uploads the offsets. list_end receives the end of every list.
    int lay_out(const std::vector<uint32_t>& psize, std::vector<uint64_t>& list_end, uint64_t& bytes) {
        std::vector<uint64_t> blk_out(nblocks + 1), list_out(nlists);
        list_end.resize(nlists);
        uint64_t cursor = 0;
        for (uint64_t t = 0; t < nlists; ++t) {
            const uint64_t n = list_offsets[t + 1] - list_offsets[t], nb = (n + 127) / 128;
            const uint32_t vl = 1u + (n >= (1u << 7)) + (n >= (1u << 14)) + (n >= (1u << 21)) + (n >= (1u << 28));
            list_out[t] = cursor;
            cursor += vl + 8 * nb - 4;
            for (uint64_t b = 0; b < nb; ++b) {
                const uint64_t g = list_blk0[t] + b;
                blk_out[g] = cursor;
                cursor += (uint64_t)psize[2 * g] + psize[2 * g + 1];
            }
            list_end[t] = cursor;
        }
        blk_out[nblocks] = cursor;
        bytes = cursor;
        HIP_OK(dev.alloc(&a.out, cursor + 4096));
        HIP_OK(hipMemcpy(d_blk_out, blk_out.data(), 8 * (nblocks + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_list_out, list_out.data(), 8 * nlists, hipMemcpyHostToDevice));
        a.blk_out = d_blk_out;
        a.list_out = d_list_out;
        return DS2I_OK;
    }

    // the device-written list bytes wrapped into the block_freq_index image of that codec
    int wrap(int codec, uint64_t num_docs, uint64_t bytes, const std::vector<uint64_t>& list_end, ds2i_blob** image) {
        DS2I_TRY
        ds2i_host::bytes_t lists(bytes);
        HIP_OK(hipMemcpy(lists.data(), a.out, bytes, hipMemcpyDeviceToHost));
        ds2i_host::block_index_builder builder(codec, num_docs);
        builder.set_encoded_lists(std::move(lists), list_end);
        std::unique_ptr<ds2i_blob> blob(new ds2i_blob);
        builder.freeze(blob->data);
        *image = blob.release();
        return DS2I_OK;
        DS2I_CATCH
    }
};
// plan pass, layout, write pass of one codec over a staged collection; ms accumulates the hipEvent time of the two passes
int encode_staged(EncStage& st, int codec, uint64_t num_docs, ds2i_blob** image, double& ms) {
    const uint64_t nblocks = st.nblocks;
    auto pass = [&](int which) { return nblocks ? ds2i_launch_encode(codec, which, st.a, st.grid, nullptr) : hipSuccess; };
    // ---- plan pass (the copy of the sizes below would wait for it anyway)
    HIP_OK(timed_span(nullptr, ms, [&] { return pass(0); }));
    std::vector<uint32_t> psize(2 * nblocks);
    HIP_OK(hipMemcpy(psize.data(), st.a.psize, 8 * nblocks, hipMemcpyDeviceToHost));
    std::vector<uint64_t> list_end;
    uint64_t bytes = 0;
    STAGE_OK(st.lay_out(psize, list_end, bytes));
    // ---- write pass
    HIP_OK(timed_span(nullptr, ms, [&] { return pass(1); }));
    return st.wrap(codec, num_docs, bytes, list_end, image);
}

// ---- the Elias-Fano layouts (freq_index: opt, ef, single, uniform) over a staged collection

// ---- the partition end points of the opt layout, planned on the device (partition_kernels.hip)
// Which planner an opt encode takes when the caller does not say: the device's. The images are equal, so this is a question of time
// alone, and on the configs[1] collection the whole call is a quarter shorter with it.
constexpr bool OPT_PLAN_ON_DEVICE_BY_DEFAULT = true;
// Bytes of DP scratch (12 per posting and side) one group of lists may take when the caller does not say. Lists are planned in
// groups of consecutive lists whose scratch fits; a group holds at least one list, however long.
constexpr uint64_t PART_SCRATCH_DEFAULT = 2ull << 30;

// Every list's end points, both sides, over a staged collection whose prefix sums are in d_cum. ms accumulates the hipEvent time of
// the kernels. Inside a group the items are launched longest first: list lengths are Zipf, and the DP of one list is a chain of n
// dependent steps, so the longest list of a group is its critical path and must not start behind the short ones.
int plan_partitions_staged(EncStage& st, uint64_t num_docs, const uint64_t* d_cum, uint64_t scratch_bytes, ds2i_host::opt_partitions& out,
                           double& ms) {
    using namespace ds2i_host;
    const uint64_t nlists = st.nlists;
    const uint64_t* offs = st.list_offsets;
    for (int side = 0; side < 2; ++side) {
        out.offs[side].assign(nlists + 1, 0);
        out.ends[side].clear();
    }
    if (!nlists) return DS2I_OK;
    if (nlists >= (1ull << 30)) return ds2i_set_error(DS2I_EINVAL, "more than 2^30 lists");
    if (!scratch_bytes) scratch_bytes = PART_SCRATCH_DEFAULT;
    const partition_config conf;
    const global_parameters params;
    // the budgets of the cost classes: the DP's only floating point, by the host planner's own expression (both sides cost one
    // element the same: fix_cost)
    const std::vector<uint64_t> budget = partition_budgets(partition_cost<false>(params, 1, 1, conf.fix_cost), ~uint64_t(0), conf.eps1, conf.eps2);
    if (budget.size() > ds2i_dev::PART_MAX_CLASSES) return ds2i_set_error(DS2I_EINVAL, "too many cost classes for the device planner");
    auto slots_of = [&](uint64_t t) { return 2 * (offs[t + 1] - offs[t] + 1); }; // dist / parent slots of list t, both sides
    std::vector<uint64_t> group_end;
    uint64_t max_slots = 0, max_lists = 0;
    for (uint64_t t = 0; t < nlists;) {
        uint64_t slots = slots_of(t), t1 = t + 1;
        while (t1 < nlists && (slots + slots_of(t1)) * 12 <= scratch_bytes) slots += slots_of(t1++);
        group_end.push_back(t1);
        max_slots = std::max(max_slots, slots);
        max_lists = std::max(max_lists, t1 - t);
        t = t1;
    }
    ds2i_dev::PartArgs a{};
    ds2i_dev::PartItem* d_items = nullptr;
    uint64_t *d_budget = nullptr, *d_out_offs = nullptr;
    HIP_OK(st.dev.alloc(&a.dist, 8 * max_slots));
    HIP_OK(st.dev.alloc(&a.parent, 4 * max_slots));
    HIP_OK(st.dev.alloc(&d_items, sizeof(ds2i_dev::PartItem) * 2 * max_lists));
    HIP_OK(st.dev.alloc(&d_budget, 8 * budget.size()));
    HIP_OK(st.dev.alloc(&a.count, 4 * 2 * nlists));
    HIP_OK(st.dev.alloc(&d_out_offs, 8 * 2 * (nlists + 1)));
    HIP_OK(st.dev.alloc(&a.out_ends[0], 4 * offs[nlists])); // (a list of n postings has at most n partitions)
    HIP_OK(st.dev.alloc(&a.out_ends[1], 4 * offs[nlists]));
    HIP_OK(hipMemcpy(d_budget, budget.data(), 8 * budget.size(), hipMemcpyHostToDevice));
    a.docs = st.a.docs;
    a.cum = d_cum;
    a.list_in = st.a.list_in;
    a.nlists = nlists;
    a.num_docs = num_docs;
    a.items = d_items;
    a.budget = d_budget;
    a.nbudgets = (uint32_t)budget.size();
    a.fix_cost = conf.fix_cost;
    a.out_offs = d_out_offs;
    std::vector<ds2i_dev::PartItem> items;
    std::vector<uint64_t> order;
    std::vector<uint32_t> count;
    for (uint64_t t0 = 0, g = 0; g < group_end.size(); t0 = group_end[g++]) {
        const uint64_t t1 = group_end[g], nl = t1 - t0;
        order.resize(nl);
        for (uint64_t k = 0; k < nl; ++k) order[k] = t0 + k;
        std::stable_sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return offs[x + 1] - offs[x] > offs[y + 1] - offs[y]; });
        items.clear();
        uint64_t base = 0;
        for (uint64_t t : order)
            for (uint32_t side = 0; side < 2; ++side) {
                items.push_back(ds2i_dev::PartItem{(uint32_t)t, side, base});
                base += offs[t + 1] - offs[t] + 1;
            }
        HIP_OK(hipMemcpy(d_items, items.data(), sizeof(ds2i_dev::PartItem) * items.size(), hipMemcpyHostToDevice));
        a.nitems = (uint32_t)items.size();
        HIP_OK(timed_span(nullptr, ms, [&] { return ds2i_launch_partition_plan(a, nullptr); }));
        // the counts of the group's lists -> where their end points go
        count.resize(nl);
        for (int side = 0; side < 2; ++side) {
            HIP_OK(hipMemcpy(count.data(), a.count + side * nlists + t0, 4 * nl, hipMemcpyDeviceToHost));
            for (uint64_t k = 0; k < nl; ++k) {
                if (!count[k] || count[k] > offs[t0 + k + 1] - offs[t0 + k]) return ds2i_set_error(DS2I_EFORMAT, "the device planner returned an impossible partition count");
                out.offs[side][t0 + k + 1] = out.offs[side][t0 + k] + count[k];
            }
            HIP_OK(hipMemcpy(d_out_offs + side * (nlists + 1) + t0, out.offs[side].data() + t0, 8 * (nl + 1), hipMemcpyHostToDevice));
        }
        HIP_OK(timed_span(nullptr, ms, [&] { return ds2i_launch_partition_gather(a, nullptr); }));
    }
    for (int side = 0; side < 2; ++side) {
        out.ends[side].resize(out.offs[side][nlists]);
        HIP_OK(hipMemcpy(out.ends[side].data(), a.out_ends[side], 4 * out.ends[side].size(), hipMemcpyDeviceToHost));
    }
    return DS2I_OK;
}

// the 64-bit prefix sums of every list's freqs (positive_sequence), left in *d_cum
int prefix_sums_staged(EncStage& st, uint64_t** d_cum, double& ms) {
    uint64_t* d_blk_base = nullptr;
    HIP_OK(st.dev.alloc(&d_blk_base, 8 * st.nblocks));
    HIP_OK(st.dev.alloc(d_cum, 8 * st.list_offsets[st.nlists]));
    HIP_OK(timed_span(nullptr, ms, [&] {
        return st.nblocks ? ds2i_launch_freq_prefix_sums(st.a, st.nlists, d_blk_base, *d_cum, st.grid, nullptr) : hipSuccess;
    }));
    return DS2I_OK;
}

// how an opt encode plans its partitions: DS2I_ENCODE_PLAN_* of ds2i_hip.h, 0 = the default
int plan_on_device(const char* who, uint32_t flags, bool& device) {
    if ((flags & DS2I_ENCODE_PLAN_HOST) && (flags & DS2I_ENCODE_PLAN_DEVICE))
        return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": both planners asked for").c_str());
    device = (flags & DS2I_ENCODE_PLAN_DEVICE) || (!(flags & DS2I_ENCODE_PLAN_HOST) && OPT_PLAN_ON_DEVICE_BY_DEFAULT);
    return DS2I_OK;
}

// Plan (for opt: the partition end points, by optimal_partition list-parallel on the host or by the device planner; then headers
// and jobs on the host), prefix sums and base sequences on the device, headers ORed into the downloaded vectors,
// opt_index_builder::freeze around them. ms accumulates the hipEvent time of the kernels; the host's two phases are left in
// freq_host_s for ds2i_hip_encode_host_seconds, the partition kernels' time in freq_plan_ms for ds2i_hip_encode_plan_ms.
thread_local double freq_host_s[2] = {0.0, 0.0}; // seconds of {planning, download + headers + freeze} of this thread's last call
thread_local double freq_plan_ms = 0.0;          // hipEvent time of the partition kernels of this thread's last call
int freq_encode_staged(EncStage& st, int layout, uint64_t num_docs, const uint32_t* docs, const uint32_t* freqs, bool device_plan,
                       ds2i_blob** image, double& ms) {
    using namespace ds2i_host;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t nlists = st.nlists;
    const uint64_t* offs = st.list_offsets;
    const uint64_t postings = offs[nlists];
    const global_parameters params;
    // ---- device: the prefix sums of the freqs, which the device planner and the writer share
    uint64_t* d_cum = nullptr;
    double plan_phase_ms = 0.0; // kernel time inside the planning phase: not the host's
    STAGE_OK(prefix_sums_staged(st, &d_cum, plan_phase_ms));
    opt_partitions parts;
    device_plan = device_plan && layout == LAYOUT_OPT;
    if (device_plan) {
        STAGE_OK(plan_partitions_staged(st, num_docs, d_cum, 0, parts, freq_plan_ms));
        plan_phase_ms += freq_plan_ms;
    }
    ms += plan_phase_ms;
    std::vector<freq_list_plan> plans(nlists);
    const unsigned threads = plan_threads(nlists);
    parallel_for(nlists, threads, [&](uint64_t t, unsigned) {
        if (device_plan) {
            const std::vector<uint32_t> de = parts.of(0, t), fe = parts.of(1, t);
            plan_list(layout, num_docs, params, offs[t], offs[t + 1] - offs[t], docs + offs[t], freqs + offs[t], plans[t], &de, &fe);
        } else {
            plan_list(layout, num_docs, params, offs[t], offs[t + 1] - offs[t], docs + offs[t], freqs + offs[t], plans[t]);
        }
    }, true);
    // where every list starts in the two bit vectors; the jobs move to their final offsets
    std::vector<uint64_t> ends[2], head_at[2];
    std::vector<ds2i_dev::FreqJob> jobs[2];
    for (int side = 0; side < 2; ++side) {
        uint64_t njobs = 0;
        for (auto const& pl : plans) njobs += pl.jobs[side].size();
        jobs[side].reserve(njobs);
        ends[side].assign(1, 0);
        ends[side].reserve(nlists + 1);
        uint64_t cursor = 0;
        for (auto& pl : plans) {
            const uint64_t body_at = cursor + pl.head[side].size();
            for (auto j : pl.jobs[side]) {
                place(j, body_at);
                jobs[side].push_back(j);
            }
            std::vector<ds2i_dev::FreqJob>().swap(pl.jobs[side]);
            cursor = body_at + pl.body_bits[side];
            ends[side].push_back(cursor);
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    // ---- device: the base sequences of both sides
    ds2i_dev::FreqEncArgs fa[2];
    uint64_t words[2];
    for (int side = 0; side < 2; ++side) {
        ds2i_dev::FreqJob* d_jobs = nullptr;
        unsigned long long* d_out = nullptr;
        words[side] = (ends[side].back() + 63) / 64;
        HIP_OK(st.dev.alloc(&d_jobs, sizeof(ds2i_dev::FreqJob) * jobs[side].size()));
        HIP_OK(st.dev.alloc(&d_out, 8 * (words[side] + 2)));
        HIP_OK(hipMemcpy(d_jobs, jobs[side].data(), sizeof(ds2i_dev::FreqJob) * jobs[side].size(), hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0, 8 * (words[side] + 2)));
        fa[side].docs = st.a.docs;
        fa[side].cum = d_cum;
        fa[side].jobs = d_jobs;
        fa[side].njobs = jobs[side].size();
        fa[side].postings = postings;
        fa[side].out = d_out;
        fa[side].nbits = ends[side].back();
        std::vector<ds2i_dev::FreqJob>().swap(jobs[side]);
    }
    HIP_OK(timed_span(nullptr, ms, [&] {
        if (!st.nblocks) return hipSuccess;
        hipError_t e = ds2i_launch_freq_write(0, fa[0], st.grid, nullptr);
        if (e == hipSuccess) e = ds2i_launch_freq_write(1, fa[1], st.grid, nullptr);
        return e;
    }));
    // ---- host: the headers join the device's words; the container is the host builder's
    const auto t2 = std::chrono::steady_clock::now();
    DS2I_TRY
    bitvec_builder bits[2];
    for (int side = 0; side < 2; ++side) {
        bits[side].zero_extend(ends[side].back());
        HIP_OK(hipMemcpy(bits[side].words().data(), fa[side].out, 8 * words[side], hipMemcpyDeviceToHost));
        for (uint64_t l = 0; l < nlists; ++l) or_bits_at(bits[side].words(), ends[side][l], plans[l].head[side]);
    }
    std::vector<freq_list_plan>().swap(plans);
    opt_index_builder builder(num_docs, params, layout);
    builder.set_encoded(std::move(bits[0]), std::move(ends[0]), std::move(bits[1]), std::move(ends[1]));
    std::unique_ptr<ds2i_blob> blob(new ds2i_blob);
    builder.freeze(blob->data);
    *image = blob.release();
    DS2I_CATCH
    freq_host_s[0] = std::chrono::duration<double>(t1 - t0).count() - 1e-3 * plan_phase_ms;
    freq_host_s[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t2).count();
    return DS2I_OK;
}

// max_term_weight of every list of a staged collection (wand_kernels.hip); ms accumulates the kernel's hipEvent time
int wand_max_staged(EncStage& st, const std::vector<float>& norm_lens, std::vector<float>& max_w, double& ms) {
    static_assert(sizeof(float) == sizeof(unsigned int), "the list maxima travel as the bits of a float");
    float* d_norm = nullptr;
    unsigned int* d_max = nullptr;
    HIP_OK(st.dev.alloc(&d_norm, 4 * norm_lens.size()));
    HIP_OK(st.dev.alloc(&d_max, 4 * st.nlists));
    HIP_OK(hipMemcpy(d_norm, norm_lens.data(), 4 * norm_lens.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_max, 0, 4 * st.nlists));
    HIP_OK(timed_span(nullptr, ms, [&] {
        return st.nblocks ? ds2i_launch_wand_list_max(st.a.docs, st.a.freqs, st.a.list_in, st.a.blk_list, st.a.list_blk0, st.a.nblocks, d_norm,
                                                      norm_lens.size(), d_max, st.grid, nullptr)
                          : hipSuccess;
    }));
    max_w.resize(st.nlists);
    HIP_OK(hipMemcpy(max_w.data(), d_max, 4 * st.nlists, hipMemcpyDeviceToHost));
    return DS2I_OK;
}

// The images of one staged collection: the index of `codec` (a block codec_kind or a freq_layout; index_image non-null) and / or the wand_data image over
// `norm_lens` (wand_image non-null), from ONE upload. Neither output is touched unless both succeed.
int build_images(const char* who, int device, int codec, uint64_t num_docs, const std::vector<float>* norm_lens, uint64_t nlists,
                 const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs, ds2i_blob** index_image,
                 ds2i_blob** wand_image, double* device_ms, uint32_t plan_flags = 0) {
    bool device_plan = false;
    STAGE_OK(plan_on_device(who, plan_flags, device_plan));
    freq_plan_ms = 0.0;
    EncStage st;
    STAGE_OK(st.upload(who, device, nlists, list_offsets, docs, freqs));
    double ms = 0.0;
    ds2i_blob* ib = nullptr;
    if (index_image)
        STAGE_OK(ds2i_host::is_freq_layout(codec) ? freq_encode_staged(st, codec, num_docs, docs, freqs, device_plan, &ib, ms)
                                                  : encode_staged(st, codec, num_docs, &ib, ms));
    std::unique_ptr<ds2i_blob> index_blob(ib), wand_blob;
    if (wand_image) {
        std::vector<float> max_w;
        STAGE_OK(wand_max_staged(st, *norm_lens, max_w, ms));
        wand_blob.reset(new ds2i_blob);
        ds2i_host::wand_freeze(*norm_lens, max_w, wand_blob->data);
    }
    if (index_image) *index_image = index_blob.release();
    if (wand_image) *wand_image = wand_blob.release();
    if (device_ms) *device_ms = ms;
    return DS2I_OK;
}

// the encoder's name for an index kind: the block codec_kind (host_encode.hpp) or the freq_layout (host_pef.hpp)
int encoder_kind_of(const char* who, int index_kind, int& codec) {
    if (ds2i_host::is_freq_layout(index_kind)) {
        static_assert(DS2I_OPT == ds2i_host::LAYOUT_OPT && DS2I_EF == ds2i_host::LAYOUT_EF && DS2I_SINGLE == ds2i_host::LAYOUT_SINGLE &&
                          DS2I_UNIFORM == ds2i_host::LAYOUT_UNIFORM, "freq_layout is numbered like ds2i_hip_index_kind");
        codec = index_kind;
        return DS2I_OK;
    }
    if (index_kind != DS2I_BLOCK_OPTPFOR && index_kind != DS2I_BLOCK_VARINT && index_kind != DS2I_BLOCK_INTERPOLATIVE)
        return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": the GPU encoder writes block_optpfor, block_varint, block_interpolative, opt, ef, "
                                                               "single and uniform indexes").c_str());
    codec = index_kind == DS2I_BLOCK_OPTPFOR ? ds2i_host::CODEC_OPTPFOR
            : index_kind == DS2I_BLOCK_VARINT ? ds2i_host::CODEC_VARINT : ds2i_host::CODEC_INTERPOLATIVE;
    return DS2I_OK;
}

// what the wand kernel's gather relies on, checked before anything is staged: no empty list (the host builder's "List
// must be nonempty", block_freq_index.hpp:31) and no doc-id past norm_lens
int check_postings(const char* who, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs) {
    for (uint64_t t = 0; t < nlists; ++t) {
        if (offs[t + 1] <= offs[t]) return ds2i_set_error(DS2I_EINVAL, "List must be nonempty");
        uint32_t top = 0;
        for (uint64_t i = offs[t]; i < offs[t + 1]; ++i) top = std::max(top, docs[i]);
        if (top >= num_docs) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": doc id out of range").c_str());
    }
    return DS2I_OK;
}
// what the Elias-Fano layouts rely on (host_freq_plan.hpp: freq_postings_fault), checked before anything is staged
int check_freq_postings(const char* who, uint64_t num_docs, uint64_t nlists, const uint64_t* offs, const uint32_t* docs,
                        const uint32_t* freqs) {
    const std::string fault = ds2i_host::freq_postings_fault(who, num_docs, nlists, offs, docs, freqs);
    return fault.empty() ? DS2I_OK : ds2i_set_error(DS2I_EINVAL, fault.c_str());
}
} // namespace

namespace {
int encode_index(const char* who, int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                 const uint32_t* docs, const uint32_t* freqs, uint32_t flags, ds2i_blob** image, double* device_ms) {
    if (!list_offsets || !docs || !freqs || !image) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": null argument").c_str());
    bool device_plan = false;
    STAGE_OK(plan_on_device(who, flags, device_plan));
    int codec = 0;
    STAGE_OK(encoder_kind_of(who, index_kind, codec));
    if (ds2i_host::is_freq_layout(codec)) STAGE_OK(check_freq_postings(who, num_docs, nlists, list_offsets, docs, freqs));
    DS2I_TRY
    return build_images(who, device, codec, num_docs, nullptr, nlists, list_offsets, docs, freqs, image, nullptr, device_ms, flags);
    DS2I_CATCH
}
} // namespace

extern "C" int ds2i_hip_encode_index(int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                                     const uint32_t* docs, const uint32_t* freqs, ds2i_blob** image, double* device_ms) {
    return encode_index("ds2i_hip_encode_index", device, index_kind, num_docs, nlists, list_offsets, docs, freqs, 0, image, device_ms);
}

extern "C" int ds2i_hip_encode_index_with(int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                                          const uint32_t* docs, const uint32_t* freqs, uint32_t flags, ds2i_blob** image, double* device_ms) {
    return encode_index("ds2i_hip_encode_index_with", device, index_kind, num_docs, nlists, list_offsets, docs, freqs, flags, image, device_ms);
}

extern "C" void ds2i_hip_encode_plan_ms(double* ms) {
    if (ms) *ms = freq_plan_ms;
}

extern "C" int ds2i_hip_opt_partition(int device, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets, const uint32_t* docs,
                                      const uint32_t* freqs, uint64_t scratch_bytes, ds2i_blob** docs_ends, ds2i_blob** docs_offs,
                                      ds2i_blob** freqs_ends, ds2i_blob** freqs_offs, double* device_ms) {
    if (!list_offsets || !docs || !freqs || !docs_ends || !docs_offs || !freqs_ends || !freqs_offs)
        return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_opt_partition: null argument");
    STAGE_OK(check_freq_postings("ds2i_hip_opt_partition", num_docs, nlists, list_offsets, docs, freqs));
    DS2I_TRY
    EncStage st;
    STAGE_OK(st.upload("ds2i_hip_opt_partition", device, nlists, list_offsets, docs, freqs));
    double prefix_ms = 0.0, ms = 0.0;
    uint64_t* d_cum = nullptr;
    STAGE_OK(prefix_sums_staged(st, &d_cum, prefix_ms));
    ds2i_host::opt_partitions parts;
    STAGE_OK(plan_partitions_staged(st, num_docs, d_cum, scratch_bytes, parts, ms));
    partition_blobs(parts, docs_ends, docs_offs, freqs_ends, freqs_offs);
    if (device_ms) *device_ms = prefix_ms + ms;
    return DS2I_OK;
    DS2I_CATCH
}

// capi_util.hpp: what ds2i_hip_convert_index asks of the encoder
int ds2i_check_encoder_kind(const char* who, int index_kind) {
    int codec = 0;
    return encoder_kind_of(who, index_kind, codec);
}

int ds2i_encode_device_postings(const char* who, int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                                uint32_t* d_docs, uint32_t* d_freqs, ds2i_blob** image, double* device_ms) {
    return ds2i_build_device_postings(who, device, index_kind, num_docs, nlists, list_offsets, d_docs, d_freqs, nullptr, image, nullptr, device_ms);
}

int ds2i_build_device_postings(const char* who, int device, int index_kind, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                               uint32_t* d_docs, uint32_t* d_freqs, const uint32_t* doc_sizes, ds2i_blob** image, ds2i_blob** wand_image,
                               double* device_ms) {
    DS2I_TRY
    freq_plan_ms = 0.0;
    EncStage st;
    const int adopted = st.adopt(who, device, nlists, list_offsets, d_docs, d_freqs);
    int codec = 0;
    STAGE_OK(encoder_kind_of(who, index_kind, codec));
    STAGE_OK(adopted);
    double ms = 0.0;
    ds2i_blob* ib = nullptr;
    if (ds2i_host::is_freq_layout(codec)) {
        // the host writes the headers from the postings: they come down once, and the base sequences are written from the device copy
        const uint64_t total = list_offsets[nlists];
        std::vector<uint32_t> docs(total ? total : 1), freqs(total ? total : 1);
        HIP_OK(hipMemcpy(docs.data(), d_docs, 4 * total, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(freqs.data(), d_freqs, 4 * total, hipMemcpyDeviceToHost));
        STAGE_OK(check_freq_postings(who, num_docs, nlists, list_offsets, docs.data(), freqs.data()));
        STAGE_OK(freq_encode_staged(st, codec, num_docs, docs.data(), freqs.data(), OPT_PLAN_ON_DEVICE_BY_DEFAULT, &ib, ms));
    } else {
        STAGE_OK(encode_staged(st, codec, num_docs, &ib, ms));
    }
    std::unique_ptr<ds2i_blob> index_blob(ib), wand_blob;
    if (wand_image) { // the wand data over the same staging, as build_images makes it
        std::vector<float> norm_lens, max_w;
        ds2i_host::compute_norm_lens(doc_sizes, num_docs, norm_lens);
        STAGE_OK(wand_max_staged(st, norm_lens, max_w, ms));
        wand_blob.reset(new ds2i_blob);
        ds2i_host::wand_freeze(norm_lens, max_w, wand_blob->data);
        *wand_image = wand_blob.release();
    }
    *image = index_blob.release();
    if (device_ms) *device_ms = ms;
    return DS2I_OK;
    DS2I_CATCH
}

extern "C" void ds2i_hip_encode_host_seconds(double seconds[2]) {
    if (seconds) seconds[0] = freq_host_s[0], seconds[1] = freq_host_s[1];
}

extern "C" int ds2i_hip_build_wand(int device, const uint32_t* doc_sizes, uint64_t num_docs, uint64_t nlists, const uint64_t* list_offsets,
                                   const uint32_t* docs, const uint32_t* freqs, ds2i_blob** wand_image, double* device_ms) {
    if (!doc_sizes || !num_docs || !list_offsets || !docs || !freqs || !wand_image)
        return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_build_wand: bad argument");
    STAGE_OK(check_postings("ds2i_hip_build_wand", num_docs, nlists, list_offsets, docs));
    DS2I_TRY
    std::vector<float> norm_lens;
    ds2i_host::compute_norm_lens(doc_sizes, num_docs, norm_lens);
    return build_images("ds2i_hip_build_wand", device, 0, num_docs, &norm_lens, nlists, list_offsets, docs, freqs, nullptr, wand_image, device_ms);
    DS2I_CATCH
}

extern "C" int ds2i_hip_build_collection(int device, int index_kind, const uint32_t* doc_sizes, uint64_t num_docs, uint64_t nlists,
                                         const uint64_t* list_offsets, const uint32_t* docs, const uint32_t* freqs,
                                         ds2i_blob** index_image, ds2i_blob** wand_image, double* device_ms) {
    if (!list_offsets || !docs || !freqs || !index_image || (wand_image && (!doc_sizes || !num_docs)))
        return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_build_collection: bad argument");
    int codec = 0;
    STAGE_OK(encoder_kind_of("ds2i_hip_build_collection", index_kind, codec));
    STAGE_OK(check_postings("ds2i_hip_build_collection", num_docs, nlists, list_offsets, docs));
    if (ds2i_host::is_freq_layout(codec)) STAGE_OK(check_freq_postings("ds2i_hip_build_collection", num_docs, nlists, list_offsets, docs, freqs));
    DS2I_TRY
    std::vector<float> norm_lens;
    if (wand_image) ds2i_host::compute_norm_lens(doc_sizes, num_docs, norm_lens);
    return build_images("ds2i_hip_build_collection", device, codec, num_docs, &norm_lens, nlists, list_offsets, docs, freqs, index_image,
                        wand_image, device_ms);
    DS2I_CATCH
}

// ---------------------------------------------------------------- block_mixed optimiser on the device
namespace {
// the builder's lists in CSR form
int hybrid_csr(const char* who, const ds2i_host::hybrid_index_builder& hb, std::vector<uint64_t>& offs, std::vector<uint32_t>& docs,
               std::vector<uint32_t>& freqs) {
    if (hb.has_virtual()) return ds2i_set_error(DS2I_EINVAL, (std::string(who) + ": the builder holds virtual lists (ds2i_synth_build_hybrid stays on the host)").c_str());
    const uint64_t V = hb.lists();
    offs.assign(V + 1, 0);
    for (uint64_t t = 0; t < V; ++t) offs[t + 1] = offs[t] + hb.list_size(t);
    docs.resize(offs[V] ? offs[V] : 1);
    freqs.resize(offs[V] ? offs[V] : 1);
    for (uint64_t t = 0; t < V; ++t) {
        std::memcpy(docs.data() + offs[t], hb.list_docs(t), 4 * hb.list_size(t));
        std::memcpy(freqs.data() + offs[t], hb.list_freqs(t), 4 * hb.list_size(t));
    }
    return DS2I_OK;
}

// plan kernel -> records -> hulls (host): leaves the builder analysed. ms accumulates the kernel's hipEvent time.
int hybrid_analyse_on(EncStage& st, ds2i_host::hybrid_index_builder& hb, double& ms) {
    const uint64_t nblocks = st.nblocks;
    HIP_OK(st.dev.alloc(&st.a.rec, sizeof(ds2i_host::hybrid_part_rec) * 2 * nblocks));
    HIP_OK(timed_span(nullptr, ms, [&] { return nblocks ? ds2i_launch_hybrid_plan(st.a, st.grid, nullptr) : hipSuccess; }));
    std::vector<ds2i_host::hybrid_part_rec> recs(2 * nblocks);
    HIP_OK(hipMemcpy(recs.data(), st.a.rec, sizeof(ds2i_host::hybrid_part_rec) * 2 * nblocks, hipMemcpyDeviceToHost));
    hb.analyse_from_records(recs.data(), 0);
    return DS2I_OK;
}
} // namespace

extern "C" int ds2i_hip_hybrid_analyse(ds2i_hybrid* h, int device, uint64_t* min_space, uint64_t* max_space, double* device_ms) {
    if (!h) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_hybrid_analyse: null argument");
    DS2I_TRY
    ds2i_host::hybrid_index_builder& hb = *h->b;
    double ms = 0.0;
    if (hb.analysed()) {
        STAGE_OK(check_device("ds2i_hip_hybrid_analyse", device));
    } else {
        std::vector<uint64_t> offs;
        std::vector<uint32_t> docs, freqs;
        STAGE_OK(hybrid_csr("ds2i_hip_hybrid_analyse", hb, offs, docs, freqs));
        EncStage st;
        STAGE_OK(st.upload("ds2i_hip_hybrid_analyse", device, hb.lists(), offs.data(), docs.data(), freqs.data()));
        STAGE_OK(hybrid_analyse_on(st, hb, ms));
    }
    if (min_space) *min_space = hb.min_space();
    if (max_space) *max_space = hb.max_space();
    if (device_ms) *device_ms = ms;
    return DS2I_OK;
    DS2I_CATCH
}

extern "C" int ds2i_hip_hybrid_freeze(ds2i_hybrid* h, int device, uint64_t budget_bytes, ds2i_blob** image, double* rate,
                                      uint64_t* space, double* model_time, uint64_t type_counts[6], double* device_ms) {
    if (!h || !image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_hybrid_freeze: null argument");
    DS2I_TRY
    ds2i_host::hybrid_index_builder& hb = *h->b;
    double ms = 0.0;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> docs, freqs;
    STAGE_OK(hybrid_csr("ds2i_hip_hybrid_freeze", hb, offs, docs, freqs));
    EncStage st;
    STAGE_OK(st.upload("ds2i_hip_hybrid_freeze", device, hb.lists(), offs.data(), docs.data(), freqs.data()));
    if (!hb.analysed()) STAGE_OK(hybrid_analyse_on(st, hb, ms));
    if (budget_bytes < hb.min_space()) return ds2i_set_error(DS2I_EINVAL, "budget below the smallest possible index");
    const double r = hb.solve(budget_bytes);
    uint64_t s = 0;
    double t = 0;
    hb.evaluate(r, s, t);
    // the choice of every part: (type, b) for the kernel, its bytes for the layout (a hull point's space IS the
    // size of the part in that encoding, type byte included), the counts of the full blocks
    const uint64_t nblocks = st.nblocks;
    std::vector<uint8_t> choice(4 * nblocks);
    std::vector<uint32_t> psize(2 * nblocks);
    uint64_t tc[6] = {0, 0, 0, 0, 0, 0};
    {
        uint64_t part = 0;
        uint64_t t_list = 0, left = hb.lists() ? hb.list_size(0) : 0; // postings of the current list from this block on
        hb.for_each_choice(r, [&](ds2i_host::hybrid_point const& c) {
            choice[2 * part] = c.type;
            choice[2 * part + 1] = (uint8_t)c.b;
            psize[part] = c.space;
            if (left >= ds2i_host::BLOCK) ++tc[3 * (part & 1) + c.type];
            if (part & 1) {
                left -= std::min<uint64_t>(left, ds2i_host::BLOCK);
                if (!left && ++t_list < hb.lists()) left = hb.list_size(t_list);
            }
            ++part;
        });
        if (part != 2 * nblocks) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_hybrid_freeze: the analysis does not match the lists");
    }
    uint8_t* d_choice = nullptr;
    HIP_OK(st.dev.alloc(&d_choice, 4 * nblocks));
    HIP_OK(hipMemcpy(d_choice, choice.data(), 4 * nblocks, hipMemcpyHostToDevice));
    st.a.choice = d_choice;
    std::vector<uint64_t> list_end;
    uint64_t bytes = 0;
    STAGE_OK(st.lay_out(psize, list_end, bytes));
    HIP_OK(timed_span(nullptr, ms, [&] { return nblocks ? ds2i_launch_encode(ds2i_host::CODEC_MIXED, 1, st.a, st.grid, nullptr) : hipSuccess; }));
    // the kernel reports what it wrote: it must be what the hulls promised, or the layout is wrong
    std::vector<uint32_t> wrote(2 * nblocks);
    HIP_OK(hipMemcpy(wrote.data(), st.a.psize, 8 * nblocks, hipMemcpyDeviceToHost));
    if (wrote != psize) return ds2i_set_error(DS2I_EFORMAT, "ds2i_hip_hybrid_freeze: a part was written at another size than its hull point");
    STAGE_OK(st.wrap(ds2i_host::CODEC_MIXED, hb.num_docs(), bytes, list_end, image));
    if (rate) *rate = r;
    if (space) *space = s;
    if (model_time) *model_time = t;
    if (type_counts) for (int i = 0; i < 6; ++i) type_counts[i] = tc[i];
    if (device_ms) *device_ms = ms;
    return DS2I_OK;
    DS2I_CATCH
}

// The synthetic collection (ds2i_build.h: ds2i_synth_params) generated on the host threads and encoded ON THE GPU:
// the fast index-construction path of the benchmark loop. Produces the same two images as ds2i_synth_build(...,
// DS2I_BLOCK_OPTPFOR, ...), byte for byte.
extern "C" int ds2i_hip_synth_encode(int device, const ds2i_synth_params* pp, int threads, ds2i_blob** index_image,
                                     ds2i_blob** wand_image, uint64_t* total_postings, double* generate_s, double* device_ms) {
    if (!pp || !index_image) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_synth_encode: null argument");
    using namespace ds2i_host;
    DS2I_TRY
    const synth_params p = to_params(pp);
    if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> sizes;
    synth_doc_sizes(p, sizes);
    std::vector<float> norm_lens;
    compute_norm_lens(sizes.data(), p.num_docs, norm_lens);
    std::vector<uint32_t>().swap(sizes);
    const uint32_t V = p.num_terms;
    std::vector<std::vector<uint32_t>> ld(V), lf(V);
    parallel_for(V, (unsigned)threads, [&](uint64_t t, unsigned) {
        const uint64_t n = synth_list(p, (uint32_t)t, ld[t], lf[t]);
        ld[t].resize(n);
        lf[t].resize(n);
        ld[t].shrink_to_fit();
        lf[t].shrink_to_fit();
    });
    std::vector<uint64_t> offs(V + 1, 0);
    for (uint32_t t = 0; t < V; ++t) offs[t + 1] = offs[t] + ld[t].size();
    std::vector<uint32_t> docs(offs[V] ? offs[V] : 1), freqs(offs[V] ? offs[V] : 1);
    parallel_for(V, (unsigned)threads, [&](uint64_t t, unsigned) {
        std::memcpy(docs.data() + offs[t], ld[t].data(), 4 * ld[t].size());
        std::memcpy(freqs.data() + offs[t], lf[t].data(), 4 * lf[t].size());
        std::vector<uint32_t>().swap(ld[t]);
        std::vector<uint32_t>().swap(lf[t]);
    });
    if (generate_s) *generate_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (total_postings) *total_postings = offs[V];
    // one staging for both images; max_term_weight comes from the wand kernel (the generator's doc-ids are < num_docs)
    STAGE_OK(build_images("ds2i_hip_synth_encode", device, CODEC_OPTPFOR, p.num_docs, &norm_lens, V, offs.data(), docs.data(), freqs.data(),
                          index_image, wand_image, device_ms));
    return DS2I_OK;
    DS2I_CATCH
}
