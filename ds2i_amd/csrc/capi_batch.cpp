// Host implementation of include/ds2i_hip.h, query half: the batch SLOT and the kernel launches. What a batch does is decided by the
// planner (batch_plan.cpp: plan_batch, host code only); the slot carries a plan to the device. Its pinned staging block, its device
// blocks and its events are allocated once and only grow, so a serving loop (ds2i_hip_pipeline_*) pays no allocation per batch;
// everything a batch uploads travels in ONE async H2D copy, everything it returns in ONE async D2H copy, and nothing in submit()
// blocks on the device -- the host plans batch i+1 while the kernels of batch i run.
// There is NO CPU fallback: every query result comes from the HIP kernels or the call fails.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>

#include "capi_internal.hpp"
#include "launchers.hpp"

using ds2i_dev::BatchArgs;
using ds2i_dev::MergeArgs;
using ds2i_dev::QTerm;
using ds2i_dev::Stats;
using ds2i_dev::Unit;

struct ds2i_hip_batch {
    ds2i_hip_index* idx = nullptr;
    BatchPlan plan;                   // what the batch does (plan_slot); everything below carries it out
    bool instrument = true;           // collect ds2i_hip_stats counters (instrumented kernel instantiations)
    bool alt_streams = false;         // launch on the index's second set of class streams (pipeline: odd slots of small batches)
    ds2i_hip_batch* seed = nullptr;   // plan.use_seed: the ranked_and pass over the same queries (pruning floor); the slot is kept for reuse
    bool profile_on = false;          // block access profile requested (d_prof)
    unsigned int* prof_ptr = nullptr; // where instrumented runs count block decodes (the owner's d_prof; a seed borrows it)
    // prepared batches (ds2i_hip_batch_prepare) keep their query arrays: enabling the block profile re-plans the batch without the list
    // streams and the k-wide stream kernels (PlanRequest::no_list_streams / no_bigk_streams)
    std::vector<uint32_t> keep_terms, keep_offs;
    int keep_want_matches = 0;
    bool profiled_run = false; // the last launch counted block decodes: its stream groups ran the class kernels (launched_kernel)
    DevBuf d_up, d_out, d_scr, d_matches, d_prof, d_stats, d_long, d_clk;
    PinBuf h_up, h_out;
    hipEvent_t ev_up = nullptr, ev_clear = nullptr, ev_done = nullptr, ev_c0[NCLS] = {}, ev_c1[NCLS] = {};
    // a class may run several kernels back to back (ranked_and: one per exact list count): hipEvents around each launch group
    std::vector<hipEvent_t> ev_g[NCLS];
    std::vector<float> grp_ms[NCLS];
    bool uploaded = false, launched = false;
    float cls_ms[NCLS] = {};
    Stats cls_stats[NCLS] = {};
};

namespace {

int ensure_events(ds2i_hip_batch* b) {
    if (b->ev_up) return DS2I_OK;
    HIP_OK(hipEventCreate(&b->ev_up));
    HIP_OK(hipEventCreate(&b->ev_clear));
    HIP_OK(hipEventCreate(&b->ev_done));
    for (int c = 0; c < NCLS; ++c) {
        HIP_OK(hipEventCreate(&b->ev_c0[c]));
        HIP_OK(hipEventCreate(&b->ev_c1[c]));
    }
    return DS2I_OK;
}

// ---------------------------------------------------------------- plan: the slot's plan for a request, and its seed slot's
// (the planner's error becomes the library's; whatever the slot held before is neither uploaded nor launched any more)
int plan_slot(ds2i_hip_batch* b, const PlanRequest& rq) {
    b->uploaded = b->launched = false;
    if (plan_batch(b->plan, ds2i_plan_index(b->idx), rq)) return ds2i_set_error(b->plan.rc, b->plan.err.c_str());
    if (!b->plan.use_seed) return DS2I_OK;
    if (!b->seed) {
        b->seed = new ds2i_hip_batch;
        b->seed->idx = b->idx;
    }
    return plan_slot(b->seed, seed_request(b->plan));
}

// dwords of global scratch per unit of the long class (k_daat_long: the enumerator state and the current block of every list)
size_t long_stride(const ds2i_hip_batch* b) { return (size_t)b->plan.long_terms * (256 + ds2i_meta_words() + 2) + 16; }

// ---------------------------------------------------------------- upload: one async H2D copy of the packed plan
int upload_batch(ds2i_hip_batch* b) {
    ds2i_hip_index* idx = b->idx;
    int rc = ensure_events(b);
    if (rc) return rc;
    if (b->plan.use_seed) {
        rc = upload_batch(b->seed);
        if (rc) return rc;
    }
    HIP_OK(b->h_up.reserve(b->plan.up_bytes));
    HIP_OK(b->d_up.reserve(b->plan.up_bytes));
    HIP_OK(b->d_out.reserve(b->plan.out_bytes));
    HIP_OK(b->h_out.reserve(b->plan.out_bytes));
    HIP_OK(b->d_scr.reserve(b->plan.scr_bytes));
    HIP_OK(b->d_stats.reserve(NCLS * sizeof(Stats)));
    if (b->plan.want_matches) HIP_OK(b->d_matches.reserve(4 * (size_t)(b->plan.match_off[b->plan.nq] ? b->plan.match_off[b->plan.nq] : 1)));
    if (b->plan.long_terms) HIP_OK(b->d_long.reserve(4 * long_stride(b) * std::max<uint32_t>(1, b->plan.ncls[CLS_LONG])));
    pack_upload(b->plan, (uint8_t*)b->h_up.p);
    HIP_OK(hipMemcpyAsync(b->d_up.p, b->h_up.p, b->plan.up_bytes, hipMemcpyHostToDevice, idx->s_up));
    HIP_OK(hipEventRecord(b->ev_up, idx->s_up));
    b->uploaded = true;
    return DS2I_OK;
}

// ---------------------------------------------------------------- launch: kernels + merge + one async D2H; no host sync
// The kernel a launch group runs in this launch: the one the plan chose for it, except in a counting run (block profile on,
// instrumented: profiled_run), where a stream group runs the class kernel -- the class kernels count their block decodes
GroupKernel launched_kernel(const ds2i_hip_batch* b, const SubLaunch& sl) { return b->profiled_run ? GroupKernel::cls : sl.kernel; }

// one launch group's kernel (a.order / a.urec / a.nslice / a.dyn_lists already point at the group)
hipError_t launch_group(const ds2i_hip_batch* b, GroupKernel kernel, int c, const BatchArgs& a, hipStream_t s) {
    const int lists = (int)a.dyn_lists;
    const bool docs = b->plan.route.docs; // DS2I_OP_TOPK_DOCS: the *_docs build of the same launcher
    switch (kernel) {
    case GroupKernel::ranked_stream: return (docs ? ds2i_launch_ranked_stream_docs : ds2i_launch_ranked_stream)(lists, a, a.nslice, s);
    case GroupKernel::ranked_stream_bigk: return (docs ? ds2i_launch_ranked_stream_bigk_docs : ds2i_launch_ranked_stream_bigk)(lists, a, a.nslice, s);
    case GroupKernel::ranked_stream_mixed: return (docs ? ds2i_launch_ranked_stream_mixed_docs : ds2i_launch_ranked_stream_mixed)(lists, a, a.nslice, s);
    case GroupKernel::union_stream: return (docs ? ds2i_launch_union_stream_docs : ds2i_launch_union_stream)(lists, a, a.nslice, s);
    case GroupKernel::union_stream_bigk: return (docs ? ds2i_launch_union_stream_bigk_docs : ds2i_launch_union_stream_bigk)(lists, a, a.nslice, s);
    case GroupKernel::and_rstream:
        if (docs) return hipErrorInvalidValue; // (plan_route: the flag is for ranked operators)
        return ds2i_launch_and_rstream(lists, b->plan.route.base_op == DS2I_OP_AND_FREQ ? 1 : 0, a, a.nslice, s);
    case GroupKernel::cls: break;
    }
    const int op = !docs && b->plan.route.freq_stream ? (int)DS2I_OP_OR : (b->plan.route.base_op | (b->plan.route.reference ? (int)DS2I_OP_REFERENCE_ORDER : 0));
    return (docs ? ds2i_launch_batch_docs : ds2i_launch_batch)(op, c, a, a.nslice, s);
}

// and / and_freq of the all-dense queries: list streams beside the class kernels (nobody else writes these queries' results);
// or_freq: its freqs beside the union kernels -- nobody else writes the checksums (the union kernels and k_merge get no pointer to them).
// On the stream of the >16-term class when the batch has no such query (else on the merge stream, ahead of the merge).
int launch_list_streams(ds2i_hip_batch* b, hipStream_t* cstreams, hipStream_t sm) {
    const ds2i_hip_index* idx = b->idx;
    const bool own = b->plan.ncls[CLS_LONG] == 0;
    hipStream_t sf = own ? cstreams[CLS_LONG] : sm;
    if (own) HIP_OK(hipStreamWaitEvent(sf, b->ev_clear, 0));
    if (!b->plan.sterms.empty()) {
        const bool with_freqs = b->plan.route.base_op == DS2I_OP_AND_FREQ;
        ds2i_dev::AndStreamArgs g{};
        g.arena = idx->d_arena;
        g.skip = idx->d_skip;
        g.xslots = idx->d_xslots;
        g.xovf = idx->d_xovf;
        g.tails = idx->d_tails;
        g.rmw = idx->d_rmw;
        g.out_count = b->d_out.at<unsigned long long>(b->plan.o_count);
        g.out_freq_sum = with_freqs ? b->d_out.at<unsigned long long>(b->plan.o_freq_sum) : nullptr;
        for (size_t t0 = 0; t0 < b->plan.sterms.size(); t0 += 32768) { // (grid.y is limited to 65535)
            g.terms = b->d_up.at<ds2i_dev::StreamTerm>(b->plan.o_sterms) + t0;
            HIP_OK(ds2i_launch_and_stream(g, with_freqs ? 1 : 0, b->plan.sterm_longest, (unsigned)std::min<size_t>(32768, b->plan.sterms.size() - t0), sf));
        }
    } else {
        ds2i_dev::FreqArgs f{};
        f.arena = idx->d_arena;
        f.skip = idx->d_skip;
        f.xslots = idx->d_xslots;
        f.xovf = idx->d_xovf;
        f.tails = idx->d_tails;
        f.qterms = b->d_up.at<QTerm>(b->plan.o_qterms);
        f.qterm_q = b->d_up.at<uint32_t>(b->plan.o_qterm_q);
        f.out_freq_sum = b->d_out.at<unsigned long long>(b->plan.o_freq_sum);
        uint32_t longest = 1; // (the grid has one row per term, as wide as the longest list needs)
        for (const QTerm& t : b->plan.qterms) longest = std::max(longest, t.nblocks);
        for (size_t t0 = 0; t0 < b->plan.qterms.size(); t0 += 32768) { // (grid.y is limited to 65535)
            ds2i_dev::FreqArgs g = f;
            g.qterms += t0;
            g.qterm_q += t0;
            HIP_OK(ds2i_launch_freq_stream(g, longest, (unsigned)std::min<size_t>(32768, b->plan.qterms.size() - t0), sf));
        }
    }
    if (own) {
        HIP_OK(hipEventRecord(b->ev_c1[CLS_LONG], sf));
        HIP_OK(hipStreamWaitEvent(sm, b->ev_c1[CLS_LONG], 0));
    }
    return DS2I_OK;
}

// the kernel arguments every launch group of the batch shares (launch_batch adds the group's units and the class's counters)
BatchArgs batch_args(const ds2i_hip_batch* b, bool seed_feeds) {
    const ds2i_hip_index* idx = b->idx;
    const int base_op = b->plan.route.base_op;
    BatchArgs a{};
    a.arena = idx->d_arena;
    a.bits0 = idx->d_bits0;
    a.bits1 = idx->d_bits1;
    a.norm_lens = idx->d_norm_lens;
    a.min_norm_len = idx->min_norm_len;
    a.qterms = b->d_up.at<QTerm>(b->plan.o_qterms);
    a.q_off = b->d_up.at<uint32_t>(b->plan.o_qoff);
    a.vq_info = b->plan.route.union_stream ? b->d_up.at<uint32_t>(b->plan.o_vinfo) : nullptr;
    a.ut_first = 1u;
    a.units = b->d_up.at<Unit>(b->plan.o_units);
    a.num_docs = (uint32_t)idx->num_docs;
    a.k = b->plan.k;
    a.codec = ds2i_decode_codec(idx);
    a.unit_clock = (idx->knobs.unit_clock && b->instrument) ? (unsigned long long*)b->d_clk.p : nullptr;
    a.out_count = b->d_out.at<unsigned long long>(b->plan.o_count);
    a.out_topk = b->d_out.at<float>(b->plan.o_topk);
    a.out_topk_len = b->d_out.at<uint32_t>(b->plan.o_topk_len);
    a.out_freq_sum = b->plan.route.freq_stream ? nullptr : b->d_out.at<unsigned long long>(b->plan.o_freq_sum);
    a.out_matches = b->plan.want_matches ? (uint32_t*)b->d_matches.p : nullptr;
    a.match_off = b->plan.want_matches ? b->d_up.at<unsigned long long>(b->plan.o_match_off) : nullptr;
    a.unit_count = b->d_scr.at<unsigned long long>(b->plan.o_unit_count);
    a.unit_topk = b->d_scr.at<float>(b->plan.o_unit_topk);
    a.unit_topk_len = b->d_scr.at<uint32_t>(b->plan.o_unit_topk_len);
    a.unit_freq_sum = b->d_scr.at<unsigned long long>(b->plan.o_unit_freq_sum);
    a.seed_topk = seed_feeds ? b->seed->d_out.at<float>(b->seed->plan.o_topk) : nullptr;
    a.seed_len = seed_feeds ? b->seed->d_out.at<uint32_t>(b->seed->plan.o_topk_len) : nullptr;
    a.q_floor = (base_op == DS2I_OP_RANKED_AND || b->plan.route.union_rstream()) ? b->d_scr.at<unsigned int>(b->plan.o_qfloorw) : nullptr;
    a.q_hist = b->plan.hist ? b->d_scr.at<unsigned int>(b->plan.o_qfloor) : nullptr;
    a.q_hist_slot = b->d_up.at<uint32_t>(b->plan.o_hslot);
    a.block_profile = (b->instrument && b->profile_on) ? b->prof_ptr : nullptr;
    a.skip = idx->d_skip;
    a.bmw = idx->d_bmw;
    a.rmw = (base_op == DS2I_OP_RANKED_AND && !a.bmw) ? nullptr : idx->d_rmw;
    a.rmw_bitmaps = (a.rmw && idx->has_bitmaps) ? 1u : 0u;
    a.rmh = a.rmw ? idx->d_rmh : nullptr;
    a.xslots = idx->d_xslots;
    a.xovf = idx->d_xovf;
    a.tails = idx->d_tails;
    a.long_scratch = (uint32_t*)b->d_long.p;
    a.long_stride = (uint32_t)long_stride(b);
    if (b->plan.route.docs) {
        a.out_topk_docs = b->d_out.at<uint32_t>(b->plan.o_topk_docs);
        a.unit_topk_docs = b->d_scr.at<uint32_t>(b->plan.o_unit_topk_docs);
    }
    return a;
}

int launch_batch(ds2i_hip_batch* b) {
    ds2i_hip_index* idx = b->idx;
    if (!b->uploaded) return ds2i_set_error(DS2I_EINVAL, "batch has not been prepared");
    // a counting run launches the class kernel for a stream group (launched_kernel), and the class kernels keep DS2I_HIP_MAX_K scores:
    // at a larger k the rows would come back half written. enable_block_profile plans such batches without the k-wide streams
    // (no_bigk_streams); anything else that reaches here is refused before a kernel is enqueued
    b->profiled_run = b->instrument && b->profile_on;
    if (b->plan.k > DS2I_HIP_MAX_K)
        for (int c = 0; c < NCLS; ++c)
            for (const auto& sl : b->plan.sub[c])
                if (sl.kernel != GroupKernel::cls && launched_kernel(b, sl) == GroupKernel::cls)
                    return ds2i_set_error(DS2I_EINVAL, "block profile at k > DS2I_HIP_MAX_K: a stream launch group would run a class kernel that keeps DS2I_HIP_MAX_K scores");
    if (b->plan.use_seed) { // block-synchronous ranked_and first: its k-th score seeds the pruning floor of every unit
        b->seed->instrument = b->instrument;
        b->seed->profile_on = b->profile_on;
        b->seed->prof_ptr = b->prof_ptr;
        b->seed->alt_streams = b->alt_streams;
        int rc = launch_batch(b->seed);
        if (rc) return rc;
    }
    // per-unit partials, shared floors, result block and counters start from zero. The clears go to the upload
    // stream: they depend on nothing but the slot being free, so the class kernels of this batch can start while the
    // previous batch is still being merged
    hipStream_t sm = idx->s_merge, su = idx->s_up;
    HIP_OK(hipMemsetAsync(b->d_scr.p, 0, b->plan.scr_bytes, su));
    HIP_OK(hipMemsetAsync(b->d_out.p, 0, b->plan.out_bytes, su));
    // (DS2I_OP_TOPK_DOCS: a row no kernel writes -- an empty query -- reads as padding, 0xFFFFFFFF, like the entries past a row's length)
    if (b->plan.route.docs) HIP_OK(hipMemsetAsync(b->d_out.at<uint8_t>(b->plan.o_topk_docs), 0xFF, 4 * (size_t)b->plan.nq * b->plan.k, su));
    if (b->instrument) HIP_OK(hipMemsetAsync(b->d_stats.p, 0, NCLS * sizeof(Stats), su));
    HIP_OK(hipEventRecord(b->ev_clear, su)); // also orders this launch after the batch's upload (same stream)
    // Launch order of the class kernels (they overlap on separate streams either way; measured on the GOV2-scale
    // batch): the block-synchronous conjunctions run 3 % faster when the issue-bound <=2-list class is enqueued first,
    // the disjunctive operators 2.5 % faster when the many-list classes are.
    const int base_op = b->plan.route.base_op;
    const bool small_first = !b->plan.route.reference &&
                       (base_op == DS2I_OP_AND || base_op == DS2I_OP_AND_FREQ || base_op == DS2I_OP_RANKED_AND);
    if (idx->knobs.unit_clock && b->instrument) { // diagnostic: per-unit start / end times
        HIP_OK(b->d_clk.reserve(16 * (size_t)(b->plan.nunits ? b->plan.nunits : 1)));
        HIP_OK(hipMemsetAsync(b->d_clk.p, 0, 16 * (size_t)(b->plan.nunits ? b->plan.nunits : 1), idx->s_up));
        HIP_OK(hipStreamSynchronize(idx->s_up));
    }
    if (b->alt_streams) { // (capi_internal.hpp: the second set exists from the first small batch on)
        std::lock_guard<std::mutex> lk(idx->stream_alt_mu);
        if (!idx->stream_alt[0]) {
            int lo_pri = 0, hi_pri = 0;
            HIP_OK(hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri));
            for (int c = NCLS - 1; c >= 0; --c) // (slot 0 last: it is the "set exists" mark)
                if (!idx->stream_alt[c]) HIP_OK(hipStreamCreateWithPriority(&idx->stream_alt[c], hipStreamNonBlocking, (lo_pri + hi_pri) / 2));
        }
    }
    hipStream_t* const cstreams = b->alt_streams ? idx->stream_alt : idx->stream;
    // every class stream first waits for the upload + cleared buffers, and for the seed pass when its floors feed the kernels. (In the
    // union decomposition the seed pass only ANSWERS the one-term queries -- copied into the result block on the merge stream below --
    // and the kernels of the longer queries start beside it: waiting cost the wand batch the one-term kernel's 1.2 ms in series.)
    const bool seed_feeds = b->plan.use_seed && !b->plan.route.union_stream;
    for (int c = 0; c < NCLS; ++c) {
        if (!b->plan.ncls[c]) continue;
        HIP_OK(hipStreamWaitEvent(cstreams[c], b->ev_clear, 0));
        if (seed_feeds) HIP_OK(hipStreamWaitEvent(cstreams[c], b->seed->ev_done, 0));
    }
    HIP_OK(hipStreamWaitEvent(sm, b->ev_clear, 0));
    if (b->plan.use_seed) HIP_OK(hipStreamWaitEvent(sm, b->seed->ev_done, 0));
    if (!b->plan.sterms.empty() || (b->plan.route.freq_stream && !b->plan.qterms.empty())) {
        int rc = launch_list_streams(b, cstreams, sm);
        if (rc) return rc;
    }
    // Two launch groups leave their class stream for the stream of a class this batch has no queries in (no further hardware queue is
    // opened; spreading EVERY second group that way was measured and lost): ranked_and's one-term queries (the class kernel's group of class 0: 0.9 ms behind the two-term stream
    // kernel's 2.5 ms on that class's stream) go to a spare stream -- class 0 is one of three co-critical class streams of the step
    const bool side_group0 = base_op == DS2I_OP_RANKED_AND && !b->plan.route.reference && b->plan.ncls[0] && b->plan.sub[0].size() > 1 &&
                             launched_kernel(b, b->plan.sub[0].front()) != GroupKernel::cls;
    // ... and the second stream group of the 5-8-list class (capacity 6 behind capacity 8; wand: 3.6 ms behind 7.5 ms, and: 1.3 behind 1.8)
    hipStream_t spare[NCLS];
    int nspare = 0, next_spare = 0;
    const bool side_group2 = b->plan.ncls[2] && b->plan.sub[2].size() > 1 && launched_kernel(b, b->plan.sub[2][0]) != GroupKernel::cls &&
                             launched_kernel(b, b->plan.sub[2][1]) != GroupKernel::cls;
    if (side_group0 || side_group2)
        for (int c = NCLS - 1; c >= 0; --c)
            if (!b->plan.ncls[c]) {
                spare[nspare] = cstreams[c];
                HIP_OK(hipStreamWaitEvent(spare[nspare], b->ev_clear, 0));
                if (seed_feeds) HIP_OK(hipStreamWaitEvent(spare[nspare], b->seed->ev_done, 0));
                ++nspare;
            }
    const BatchArgs args = batch_args(b, seed_feeds);
    for (int ci = NCLS - 1; ci >= 0; --ci) {
        const int c = small_first ? NCLS - 1 - ci : ci;
        if (!b->plan.ncls[c]) continue;
        hipStream_t s = cstreams[c];
        HIP_OK(hipEventRecord(b->ev_c0[c], s));
        BatchArgs a = args;
        a.stats = (b->instrument && !b->plan.route.docs) ? b->d_stats.at<Stats>(0) + c : nullptr; // (the docs kernels are built without counters)
        const uint32_t* order_base = b->d_up.at<uint32_t>(b->plan.o_order[c]);
        const ds2i_dev::UnitRec* urec_base = c < b->plan.route.urec_classes() ? b->d_up.at<ds2i_dev::UnitRec>(b->plan.o_urec[c]) : nullptr;
        for (const auto& sl : b->plan.sub[c]) { // one launch per group of the class (a single group for everything but the union kernels)
            a.order = order_base + sl.begin;
            a.urec = urec_base ? urec_base + sl.begin : nullptr;
            a.nslice = sl.end - sl.begin;
            a.dyn_lists = sl.lists;
            // (the groups of a class run back to back on its stream: launching them beside each other on further streams
            // was tried -- with that many streams the hardware queues are oversubscribed and steps of 0.5-0.9 s appear)
            const size_t gi = (size_t)(&sl - &b->plan.sub[c].front());
            while (b->ev_g[c].size() < 2 * (gi + 1)) {
                hipEvent_t e = nullptr;
                HIP_OK(hipEventCreate(&e));
                b->ev_g[c].push_back(e);
            }
            const GroupKernel kernel = launched_kernel(b, sl);
            hipStream_t sg = (gi > 0 && nspare && ((c == 0 && side_group0 && kernel == GroupKernel::cls) || (c == 2 && side_group2 && gi == 1))) ? spare[next_spare++ % nspare] : s;
            HIP_OK(hipEventRecord(b->ev_g[c][2 * gi], sg));
            HIP_OK(launch_group(b, kernel, c, a, sg));
            HIP_OK(hipEventRecord(b->ev_g[c][2 * gi + 1], sg));
            if (sg != s) HIP_OK(hipStreamWaitEvent(sm, b->ev_g[c][2 * gi + 1], 0));
        }
        HIP_OK(hipEventRecord(b->ev_c1[c], s));
        HIP_OK(hipStreamWaitEvent(sm, b->ev_c1[c], 0));
    }
    if (b->plan.nsplit) {
        MergeArgs m{};
        m.split_queries = b->d_up.at<uint32_t>(b->plan.o_split);
        m.nsplit = b->plan.nsplit;
        m.q_unit_off = b->d_up.at<uint32_t>(b->plan.o_q_unit_off);
        m.k = b->plan.k;
        m.ranked = b->plan.route.ranked;
        m.unit_count = b->d_scr.at<unsigned long long>(b->plan.o_unit_count);
        m.unit_topk = b->d_scr.at<float>(b->plan.o_unit_topk);
        m.unit_topk_len = b->d_scr.at<uint32_t>(b->plan.o_unit_topk_len);
        m.unit_freq_sum = b->d_scr.at<unsigned long long>(b->plan.o_unit_freq_sum);
        m.out_count = b->d_out.at<unsigned long long>(b->plan.o_count);
        m.out_topk = b->d_out.at<float>(b->plan.o_topk);
        m.out_topk_len = b->d_out.at<uint32_t>(b->plan.o_topk_len);
        m.out_freq_sum = b->plan.route.freq_stream ? nullptr : b->d_out.at<unsigned long long>(b->plan.o_freq_sum);
        if (b->plan.route.docs) {
            m.unit_topk_docs = b->d_scr.at<uint32_t>(b->plan.o_unit_topk_docs);
            m.out_topk_docs = b->d_out.at<uint32_t>(b->plan.o_topk_docs);
        }
        HIP_OK((b->plan.route.docs ? ds2i_launch_merge_docs : ds2i_launch_merge)(m, std::min<unsigned>(b->plan.nsplit, 4096u), sm));
    }
    if (b->plan.use_seed && b->plan.nsingle) {
        const ds2i_dev::CopySeedArgs cs{b->d_up.at<uint32_t>(b->plan.o_single), b->plan.nsingle, b->plan.k, b->seed->d_out.at<float>(b->seed->plan.o_topk),
                                        b->seed->d_out.at<uint32_t>(b->seed->plan.o_topk_len), b->seed->d_out.at<unsigned long long>(b->seed->plan.o_count),
                                        b->d_out.at<float>(b->plan.o_topk), b->d_out.at<uint32_t>(b->plan.o_topk_len), b->d_out.at<unsigned long long>(b->plan.o_count)};
        if (b->plan.route.docs)
            HIP_OK(ds2i_launch_copy_seed_docs(ds2i_dev::CopySeedDocsArgs{cs, b->seed->d_out.at<uint32_t>(b->seed->plan.o_topk_docs), b->d_out.at<uint32_t>(b->plan.o_topk_docs)}, sm));
        else
            HIP_OK(ds2i_launch_copy_seed(cs, sm));
    }
    HIP_OK(hipMemcpyAsync(b->h_out.p, b->d_out.p, b->plan.out_bytes, hipMemcpyDeviceToHost, sm));
    HIP_OK(hipEventRecord(b->ev_done, sm));
    b->launched = true;
    return DS2I_OK;
}

// ---------------------------------------------------------------- finish: wait for the batch, collect timings / counters
int finish_batch(ds2i_hip_batch* b, ds2i_hip_stats* stats) {
    if (!b->launched) return ds2i_set_error(DS2I_EINVAL, "batch has not been launched");
    HIP_OK(hipEventSynchronize(b->ev_done));
    if (b->plan.use_seed) { // (its kernels ran inside this batch's [ev_clear, ev_done] window: not added to kernel_ms again)
        ds2i_hip_stats ss;
        int rc = finish_batch(b->seed, &ss);
        if (rc) return rc;
    }
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, b->ev_clear, b->ev_done));
    for (int c = 0; c < NCLS; ++c) {
        b->cls_ms[c] = 0.f;
        if (b->plan.ncls[c]) HIP_OK(hipEventElapsedTime(&b->cls_ms[c], b->ev_c0[c], b->ev_c1[c]));
        b->grp_ms[c].assign(b->plan.ncls[c] ? b->plan.sub[c].size() : 0, 0.f);
        for (size_t g = 0; g < b->grp_ms[c].size() && 2 * g + 1 < b->ev_g[c].size(); ++g)
            HIP_OK(hipEventElapsedTime(&b->grp_ms[c][g], b->ev_g[c][2 * g], b->ev_g[c][2 * g + 1]));
    }
    if (b->instrument) HIP_OK(hipMemcpy(b->cls_stats, b->d_stats.p, NCLS * sizeof(Stats), hipMemcpyDeviceToHost));
    else std::memset(b->cls_stats, 0, sizeof(b->cls_stats));
    if (b->instrument && b->d_clk.p && b->idx->knobs.unit_clock) { // diagnostic: where each class kernel's time goes
        std::vector<unsigned long long> clk(2 * (size_t)b->plan.nunits);
        HIP_OK(hipMemcpy(clk.data(), b->d_clk.p, 16 * (size_t)b->plan.nunits, hipMemcpyDeviceToHost));
        for (int c = 0; c < NCLS; ++c) {
            if (!b->plan.ncls[c]) continue;
            unsigned long long t0 = ~0ull, t1 = 0;
            double busy = 0;
            std::vector<std::pair<unsigned long long, uint32_t>> durs;
            for (uint32_t uid : b->plan.order[c]) {
                const unsigned long long s0 = clk[2 * (size_t)uid], e0 = clk[2 * (size_t)uid + 1];
                if (!e0) continue;
                t0 = std::min(t0, s0);
                t1 = std::max(t1, e0);
                busy += (double)(e0 - s0);
                durs.push_back({e0 - s0, uid});
            }
            if (durs.empty()) continue;
            std::sort(durs.begin(), durs.end());
            const double tick_us = 0.01; // s_memrealtime: 100 MHz
            std::fprintf(stderr, "ds2i unit clock: class %d: %zu units, span %.0f us, sum of unit times %.0f us (= %.0f waves busy on average), median unit %.1f us, p99 %.1f us\n",
                         c, durs.size(), (t1 - t0) * tick_us, busy * tick_us, busy / (double)(t1 - t0), durs[durs.size() / 2].first * tick_us,
                         durs[durs.size() * 99 / 100].first * tick_us);
            if (b->plan.route.union_stream && !b->plan.vinfo.empty()) { // wand / maxscore / ranked_or: where the time goes by driving list (e = its exclusion lists)
                double by_e[DS2I_HIP_MAX_TERMS + 1] = {}, blocks_e[DS2I_HIP_MAX_TERMS + 1] = {};
                size_t n_e[DS2I_HIP_MAX_TERMS + 1] = {};
                for (const auto& d : durs) {
                    const Unit& u = b->plan.units[d.second];
                    const uint32_t e = std::min<uint32_t>(b->plan.vinfo[3 * (size_t)u.q + 1], DS2I_HIP_MAX_TERMS);
                    by_e[e] += (double)d.first;
                    blocks_e[e] += (double)(u.blk_end - u.blk_begin);
                    ++n_e[e];
                }
                for (uint32_t e = 0; e <= DS2I_HIP_MAX_TERMS; ++e)
                    if (n_e[e]) std::fprintf(stderr, "    driving list %u: %zu units of %.0f blocks, %.0f us of unit time (%.1f us per owned block)\n", e, n_e[e], blocks_e[e], by_e[e] * tick_us,
                                             by_e[e] * tick_us / std::max(1.0, blocks_e[e]));
            }
            for (size_t i = 0; i < 8 && i < durs.size(); ++i) {
                const auto& d = durs[durs.size() - 1 - i];
                const Unit& u = b->plan.units[d.second];
                std::fprintf(stderr, "    unit %u: query %u part [%u, %u) of %u parts, %.0f us, started at +%.0f us, ended at +%.0f us\n", d.second, u.q, u.blk_begin,
                             u.blk_end, u.nparts, d.first * tick_us, (clk[2 * (size_t)d.second] - t0) * tick_us, (clk[2 * (size_t)d.second + 1] - t0) * tick_us);
            }
        }
    }
    if (stats) {
        stats->kernel_ms = ms;
        stats->docs_blocks_decoded = stats->freqs_blocks_decoded = stats->block_max_examined = 0;
        stats->algorithmic_bytes = stats->postings_scored = stats->rounds = 0;
        for (int c = 0; c < NCLS; ++c) {
            stats->docs_blocks_decoded += b->cls_stats[c].docs_blocks;
            stats->freqs_blocks_decoded += b->cls_stats[c].freqs_blocks;
            stats->block_max_examined += b->cls_stats[c].block_max_examined;
            stats->algorithmic_bytes += b->cls_stats[c].algorithmic_bytes;
            stats->postings_scored += b->cls_stats[c].postings_scored;
            stats->rounds += b->cls_stats[c].rounds;
        }
    }
    return DS2I_OK;
}

// results of the last finished run, from the pinned mirror
void copy_results(const ds2i_hip_batch* b, uint64_t* out_count, float* out_topk, uint32_t* out_topk_len, uint64_t* out_freq_sum) {
    const size_t nq = b->plan.nq;
    if (!nq) return;
    const uint8_t* h = (const uint8_t*)b->h_out.p;
    const bool ranked = b->plan.route.ranked;
    if (out_count) std::memcpy(out_count, h + b->plan.o_count, 8 * nq);
    if (out_topk && ranked) std::memcpy(out_topk, h + b->plan.o_topk, 4 * nq * b->plan.k); // and / or have no top-k (k is ignored)
    if (out_topk && ranked) // (rows no kernel wrote: padded like a written row, with -inf)
        for (uint32_t q : b->plan.empty_queries) std::fill_n(out_topk + (size_t)q * b->plan.k, b->plan.k, -std::numeric_limits<float>::infinity());
    if (out_topk_len) std::memcpy(out_topk_len, h + b->plan.o_topk_len, 4 * nq);
    if (out_freq_sum) std::memcpy(out_freq_sum, h + b->plan.o_freq_sum, 8 * nq);
}
// ... and the doc-ids of a DS2I_OP_TOPK_DOCS batch
void copy_topk_docs(const ds2i_hip_batch* b, uint32_t* out_docs) {
    if (b->plan.nq && out_docs && b->plan.route.docs) std::memcpy(out_docs, (const uint8_t*)b->h_out.p + b->plan.o_topk_docs, 4 * (size_t)b->plan.nq * b->plan.k);
}

} // namespace

void ds2i_batch_destroy(ds2i_hip_batch* b) {
    if (!b) return;
    if (b->seed) ds2i_batch_destroy(b->seed);
    (void)hipSetDevice(b->idx->device);
    if (b->launched) (void)hipEventSynchronize(b->ev_done); // never free buffers under a running kernel
    if (b->ev_up) {
        (void)hipEventDestroy(b->ev_up);
        (void)hipEventDestroy(b->ev_clear);
        (void)hipEventDestroy(b->ev_done);
        for (int c = 0; c < NCLS; ++c) {
            (void)hipEventDestroy(b->ev_c0[c]);
            (void)hipEventDestroy(b->ev_c1[c]);
        }
    }
    for (auto& v : b->ev_g) for (hipEvent_t e : v) (void)hipEventDestroy(e);

    delete b; // DevBuf / PinBuf members release their memory
}

struct ds2i_hip_pipeline {
    ds2i_hip_index* idx = nullptr;
    std::vector<ds2i_hip_batch*> slots;
    std::vector<uint64_t> slot_ticket;
    std::vector<char> busy;
    uint64_t next_ticket = 0;
    ds2i_hip_batch* last_waited = nullptr;
    // (the host half of a batch -- normalisation, BM25 query weights, work-unit planning -- runs on the caller's thread, spread over
    // DS2I_PLAN_THREADS planning threads; a planner thread OF the pipeline was built in round 4, measured slower, and removed in round 6)
};

namespace {
// A launch that failed part-way may have kernels of this slot in flight (the seed pass, some class kernels) with no
// completion event recorded: wait for the device before the caller can reuse or free the slot's buffers. The error
// being reported is kept (the drain's own status is secondary).
int drain_after_failure(ds2i_hip_batch* b, int rc) {
    const std::string keep = ds2i_get_error();
    (void)hipSetDevice(b->idx->device);
    (void)hipDeviceSynchronize();
    return ds2i_set_error(rc, keep.c_str());
}

// plan + upload + launch of one slot
int pipeline_launch(ds2i_hip_pipeline* p, size_t slot, int op, uint32_t k, const uint32_t* terms, const uint32_t* offs, uint32_t nq) {
    HIP_OK(hipSetDevice(p->idx->device));
    ds2i_hip_batch* b = p->slots[slot];
    // (capi_internal.hpp, stream_alt; with the pool-sized units above, GOV2 scale: 512 queries 536 k against 367 k queries/s on one set,
    // 1024: 833 k against 601 k, wand 512: 265 k against 181 k)
    // (three sets, slot % 3: 256 queries 367 k against 403 k on two, 512: 564 k / 532 k, 1024: 831 k / 821 k, wand 512: 232 k / 261 k -- two)
    b->alt_streams = (slot & 1) != 0 && nq < 2048;
    PlanRequest rq{op, k, terms, offs, nq, 0};
    rq.pool_batches = (uint32_t)p->slots.size();
    int rc = plan_slot(b, rq);
    if (rc) return rc; // (nothing enqueued yet)
    rc = upload_batch(b);
    if (!rc) rc = launch_batch(b);
    return rc ? drain_after_failure(b, rc) : DS2I_OK; // (nothing of the slot is still running when the error is reported)
}
} // namespace

extern "C" {

void ds2i_hip_batch_free(ds2i_hip_batch* b) { ds2i_batch_destroy(b); }

int ds2i_hip_batch_prepare(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms,
                           const uint32_t* query_offsets, uint32_t nq, int want_matches, ds2i_hip_batch** out) {
    if (!idx || !out) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_prepare: null argument");
    HIP_OK(hipSetDevice(idx->device));
    std::unique_ptr<ds2i_hip_batch, void (*)(ds2i_hip_batch*)> b(new ds2i_hip_batch, ds2i_batch_destroy);
    b->idx = idx;
    int rc = plan_slot(b.get(), PlanRequest{op, k, terms, query_offsets, nq, want_matches});
    if (!rc) rc = upload_batch(b.get());
    if (rc) return rc;
    HIP_OK(hipEventSynchronize(b->ev_up));
    try {
        b->keep_offs.assign(query_offsets, query_offsets + nq + 1);
        b->keep_terms.assign(terms, terms + (nq ? query_offsets[nq] : 0));
        b->keep_want_matches = want_matches;
    } catch (std::bad_alloc const&) {
        return ds2i_set_error(DS2I_ENOMEM, "out of host memory preparing the batch");
    }
    *out = b.release();
    return DS2I_OK;
}

int ds2i_hip_batch_run(ds2i_hip_batch* b, ds2i_hip_stats* stats) {
    if (!b) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_run: null batch");
    HIP_OK(hipSetDevice(b->idx->device));
    int rc = launch_batch(b);
    if (rc) return drain_after_failure(b, rc);
    return finish_batch(b, stats);
}

// GPU-side counterpart of profile_queries.cpp: per-block decode counts of the batch (input of the block_mixed
// optimiser, ds2i_hybrid_*). Counting happens in instrumented runs only and accumulates over runs.
int ds2i_hip_batch_enable_block_profile(ds2i_hip_batch* b) {
    if (!b) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_enable_block_profile: null batch");
    ds2i_hip_index* idx = b->idx;
    if (idx->kind >= DS2I_OPT) return ds2i_set_error(DS2I_EINVAL, "the block access profile exists for block indexes only");
    if (b->plan.route.docs) return ds2i_set_error(DS2I_EINVAL, "DS2I_OP_TOPK_DOCS batches run without counters: no block access profile");
    HIP_OK(hipSetDevice(idx->device));
    const size_t bytes = 8 * (size_t)(idx->total_blocks ? idx->total_blocks : 1);
    HIP_OK(b->d_prof.reserve(bytes));
    HIP_OK(hipMemset(b->d_prof.p, 0, bytes));
    if ((!b->plan.sterms.empty() || b->plan.route.freq_stream || b->plan.k > DS2I_HIP_MAX_K) && !b->keep_offs.empty()) {
        // queries answered by list streams have no work units and their kernels count nothing: plan the batch again without them, so
        // that every block decode of the batch shows in the profile (the input of the block_mixed optimiser). At k > 64 the stream
        // groups cannot fall back to the class kernels (launch_batch): those queries go to k_daat_long, the seed pass with them
        PlanRequest rq{b->plan.op, b->plan.k, b->keep_terms.empty() ? nullptr : b->keep_terms.data(), b->keep_offs.data(), b->plan.nq, b->keep_want_matches};
        rq.no_list_streams = true;
        rq.no_bigk_streams = true;
        HIP_OK(hipDeviceSynchronize());
        int rc = plan_slot(b, rq);
        if (!rc) rc = upload_batch(b);
        if (rc) return rc;
        HIP_OK(hipEventSynchronize(b->ev_up));
    }
    b->profile_on = true;
    b->prof_ptr = (unsigned int*)b->d_prof.p; // the seed pass decodes blocks too: launch_batch hands it the same buffer
    return DS2I_OK;
}
int ds2i_hip_batch_block_profile(ds2i_hip_batch* b, uint32_t* counts, uint64_t capacity, uint64_t* total_blocks) {
    if (!b) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_block_profile: null batch");
    ds2i_hip_index* idx = b->idx;
    if (total_blocks) *total_blocks = idx->total_blocks;
    if (!counts) return DS2I_OK;
    if (!b->profile_on) return ds2i_set_error(DS2I_EINVAL, "block profile not enabled on this batch");
    if (capacity < 2 * idx->total_blocks) return ds2i_set_error(DS2I_EINVAL, "counts buffer too small (2 per block)");
    HIP_OK(hipSetDevice(idx->device));
    HIP_OK(hipMemcpy(counts, b->d_prof.p, 8 * (size_t)idx->total_blocks, hipMemcpyDeviceToHost));
    return DS2I_OK;
}

int ds2i_hip_batch_set_instrumented(ds2i_hip_batch* b, int on) {
    if (!b) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_set_instrumented: null batch");
    b->instrument = on != 0;
    return DS2I_OK;
}

int ds2i_hip_batch_class_stats(ds2i_hip_batch* b, int cls, ds2i_hip_stats* out, uint32_t* nqueries) {
    if (!b || !out || cls < 0 || cls >= NCLS) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_class_stats: bad argument");
    out->kernel_ms = b->cls_ms[cls];
    out->docs_blocks_decoded = b->cls_stats[cls].docs_blocks;
    out->freqs_blocks_decoded = b->cls_stats[cls].freqs_blocks;
    out->block_max_examined = b->cls_stats[cls].block_max_examined;
    out->algorithmic_bytes = b->cls_stats[cls].algorithmic_bytes;
    out->postings_scored = b->cls_stats[cls].postings_scored;
    out->rounds = b->cls_stats[cls].rounds;
    if (nqueries) *nqueries = b->plan.nqcls[cls];
    return DS2I_OK;
}

// the launch groups of class `cls` in the last run: hipEvent duration, list slots the group's kernel was launched with, units
// (= workgroups), queries, and whether it ran the pipelined ranked_and kernel (k_ranked_stream<lists>, ranked_stream.hip)
int ds2i_hip_batch_class_groups(ds2i_hip_batch* b, int cls, ds2i_hip_group_stats* out, uint32_t capacity, uint32_t* ngroups) {
    if (!b || !ngroups || cls < 0 || cls >= NCLS) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_class_groups: bad argument");
    const uint32_t n = b->plan.ncls[cls] ? (uint32_t)b->plan.sub[cls].size() : 0u;
    *ngroups = n;
    if (!out) return DS2I_OK;
    for (uint32_t g = 0; g < n && g < capacity; ++g) {
        const auto& sl = b->plan.sub[cls][g];
        out[g].kernel_ms = g < b->grp_ms[cls].size() ? b->grp_ms[cls][g] : 0.0;
        out[g].lists = sl.lists;
        out[g].units = sl.end - sl.begin;
        out[g].pipelined_stream = launched_kernel(b, sl) != GroupKernel::cls ? 1 : 0;
        uint32_t nq = 0; // distinct queries of the group (its units are grouped by query only loosely: count by marking)
        std::vector<char> seen(b->plan.nq ? b->plan.nq : 1, 0);
        for (uint32_t i = sl.begin; i < sl.end; ++i) {
            const uint32_t q = b->plan.route.union_stream ? 0u : b->plan.units[b->plan.order[cls][i]].q;
            if (q < seen.size() && !seen[q]) { seen[q] = 1; ++nq; }
        }
        out[g].queries = nq;
    }
    return DS2I_OK;
}

// diagnostic: phase cycle sums of class `cls` (all zero unless built with -DDS2I_PHASE_TIMING)
int ds2i_hip_batch_phase_cycles(ds2i_hip_batch* b, int cls, uint64_t* out, int n) {
    if (!b || !out || cls < 0 || cls >= NCLS) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_phase_cycles: bad argument");
    for (int i = 0; i < n && i < ds2i_dev::PH_COUNT; ++i) out[i] = b->cls_stats[cls].phase_cycles[i];
    return DS2I_OK;
}

int ds2i_hip_batch_fetch(ds2i_hip_batch* b, uint64_t* out_count, float* out_topk, uint32_t* out_topk_len,
                         uint64_t* out_freq_sum) {
    if (!b) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_fetch: null batch");
    if (!b->launched) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_fetch: the batch has not been run");
    HIP_OK(hipSetDevice(b->idx->device));
    HIP_OK(hipEventSynchronize(b->ev_done));
    copy_results(b, out_count, out_topk, out_topk_len, out_freq_sum);
    return DS2I_OK;
}

int ds2i_hip_batch_fetch_topk_docs(ds2i_hip_batch* b, uint32_t* out_docs) {
    if (!b || !out_docs) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_fetch_topk_docs: null argument");
    if (!b->plan.route.docs) return ds2i_set_error(DS2I_EINVAL, "batch was prepared without DS2I_OP_TOPK_DOCS");
    if (!b->launched) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_fetch_topk_docs: the batch has not been run");
    HIP_OK(hipSetDevice(b->idx->device));
    HIP_OK(hipEventSynchronize(b->ev_done));
    copy_topk_docs(b, out_docs);
    return DS2I_OK;
}

int ds2i_hip_batch_match_total(ds2i_hip_batch* b, uint64_t* total) {
    if (!b || !total) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_match_total: null argument");
    *total = b->plan.want_matches ? b->plan.match_off[b->plan.nq] : 0; // capacity: 128 per block of each query's shortest list
    return DS2I_OK;
}

// On return matches of query q occupy [match_offsets[q], match_offsets[q] + out_count[q]); the device
// buffer holds one segment per work unit (at 128*blk_begin), compacted here on the host.
int ds2i_hip_batch_fetch_matches(ds2i_hip_batch* b, uint64_t* match_offsets, uint32_t* matches) {
    if (!b || !match_offsets || !matches) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_fetch_matches: null argument");
    if (!b->plan.want_matches) return ds2i_set_error(DS2I_EINVAL, "batch was prepared without want_matches");
    if (!b->launched) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_batch_fetch_matches: the batch has not been run");
    HIP_OK(hipSetDevice(b->idx->device));
    HIP_OK(hipEventSynchronize(b->ev_done));
    for (size_t i = 0; i <= b->plan.nq; ++i) match_offsets[i] = b->plan.match_off[i];
    const size_t total = (size_t)b->plan.match_off[b->plan.nq];
    if (!total) return DS2I_OK;
    HIP_OK(hipMemcpy(matches, b->d_matches.p, 4 * total, hipMemcpyDeviceToHost));
    if (b->plan.nsplit) {
        std::vector<unsigned long long> ucount(b->plan.nunits);
        HIP_OK(hipMemcpy(ucount.data(), b->d_scr.at<uint8_t>(b->plan.o_unit_count), 8 * (size_t)b->plan.nunits, hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < b->plan.nq; ++q) {
            const uint32_t u0 = b->plan.q_unit_off[q], u1 = b->plan.q_unit_off[q + 1];
            if (u1 - u0 < 2) continue;
            uint32_t* base = matches + b->plan.match_off[q];
            size_t w = 0;
            for (uint32_t u = u0; u < u1; ++u) {
                const uint32_t* seg = base + 128ull * b->plan.units[u].blk_begin;
                std::memmove(base + w, seg, 4 * (size_t)ucount[u]);
                w += (size_t)ucount[u];
            }
        }
    }
    return DS2I_OK;
}

// One-shot form: the slot (pinned staging, device blocks, events) is cached in the index handle, so repeated calls
// -- the per-query latency loop of the `queries` driver, the Python op(index, terms) form -- allocate nothing.
namespace {
int query_batch_oneshot(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms, const uint32_t* query_offsets, uint32_t nq,
                        uint64_t* out_count, float* out_topk, uint32_t* out_topk_docs, uint32_t* out_topk_len, ds2i_hip_stats* stats) {
    HIP_OK(hipSetDevice(idx->device));
    if (!idx->oneshot) {
        idx->oneshot = new ds2i_hip_batch;
        idx->oneshot->idx = idx;
    }
    ds2i_hip_batch* b = idx->oneshot;
    b->profile_on = false;
    // the counters cost throughput: collected only when the caller asks for them (stats given, no DS2I_OP_NO_COUNTERS)
    b->instrument = stats != nullptr && !(op & DS2I_OP_NO_COUNTERS);
    int rc = plan_slot(b, PlanRequest{op, k, terms, query_offsets, nq, 0});
    if (!rc) rc = upload_batch(b);
    if (!rc) rc = launch_batch(b);
    if (!rc) rc = finish_batch(b, stats);
    if (!rc) copy_results(b, out_count, out_topk, out_topk_len, nullptr);
    if (!rc) copy_topk_docs(b, out_topk_docs);
    return rc;
}
} // namespace

int ds2i_hip_query_batch(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms,
                         const uint32_t* query_offsets, uint32_t nq, uint64_t* out_count, float* out_topk,
                         uint32_t* out_topk_len, ds2i_hip_stats* stats) {
    if (!idx) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_query_batch: null index");
    if (op & DS2I_OP_TOPK_DOCS) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_query_batch has no doc-id output: use ds2i_hip_query_batch_docs");
    return query_batch_oneshot(idx, op, k, terms, query_offsets, nq, out_count, out_topk, nullptr, out_topk_len, stats);
}

int ds2i_hip_query_batch_docs(ds2i_hip_index* idx, int op, uint32_t k, const uint32_t* terms, const uint32_t* query_offsets, uint32_t nq,
                              uint64_t* out_count, float* out_topk, uint32_t* out_topk_docs, uint32_t* out_topk_len, ds2i_hip_stats* stats) {
    if (!idx) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_query_batch_docs: null index");
    if (!(op & DS2I_OP_TOPK_DOCS)) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_query_batch_docs: op lacks DS2I_OP_TOPK_DOCS");
    return query_batch_oneshot(idx, op, k, terms, query_offsets, nq, out_count, out_topk, out_topk_docs, out_topk_len, stats);
}

// ---------------------------------------------------------------- pipelined form
int ds2i_hip_pipeline_create(ds2i_hip_index* idx, uint32_t depth, ds2i_hip_pipeline** out) {
    if (!idx || !out || depth == 0 || depth > 16) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_create: bad argument (depth in [1,16])");
    ds2i_hip_pipeline* p = new ds2i_hip_pipeline;
    p->idx = idx;
    for (uint32_t i = 0; i < depth; ++i) {
        ds2i_hip_batch* b = new ds2i_hip_batch;
        b->idx = idx;
        b->instrument = false;
        p->slots.push_back(b);
    }
    p->slot_ticket.assign(depth, 0);
    p->busy.assign(depth, 0);
    *out = p;
    return DS2I_OK;
}

void ds2i_hip_pipeline_destroy(ds2i_hip_pipeline* p) {
    if (!p) return;
    for (auto* b : p->slots) ds2i_batch_destroy(b);
    delete p;
}

int ds2i_hip_pipeline_submit(ds2i_hip_pipeline* p, int op, uint32_t k, const uint32_t* terms, const uint32_t* query_offsets,
                             uint32_t nq, uint64_t* ticket) {
    if (!p || !ticket) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_submit: null argument");
    const size_t slot = (size_t)(p->next_ticket % p->slots.size());
    if (p->busy[slot]) return ds2i_set_error(DS2I_EBUSY, "ds2i_hip_pipeline_submit: all slots in flight; wait for the oldest ticket first");
    {
        int rc = pipeline_launch(p, slot, op, k, terms, query_offsets, nq);
        if (rc) return rc; // the slot stays free
    }
    p->busy[slot] = 1;
    p->slot_ticket[slot] = p->next_ticket;
    *ticket = p->next_ticket++;
    return DS2I_OK;
}

int ds2i_hip_pipeline_wait_docs(ds2i_hip_pipeline* p, uint64_t ticket, uint64_t* out_count, float* out_topk, uint32_t* out_topk_docs,
                                uint32_t* out_topk_len, ds2i_hip_stats* stats) {
    if (!p) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_wait: null pipeline");
    const size_t slot = (size_t)(ticket % p->slots.size());
    if (!p->busy[slot] || p->slot_ticket[slot] != ticket)
        return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_wait: unknown or already collected ticket");
    ds2i_hip_batch* b = p->slots[slot];
    if (out_topk_docs && !b->plan.route.docs) // (before anything is collected: the ticket stays in flight)
        return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_wait_docs: the ticket was submitted without DS2I_OP_TOPK_DOCS");
    HIP_OK(hipSetDevice(p->idx->device));
    int rc = finish_batch(b, stats);
    p->busy[slot] = 0;
    if (rc) return rc;
    p->last_waited = b;
    copy_results(b, out_count, out_topk, out_topk_len, nullptr);
    copy_topk_docs(b, out_topk_docs);
    return DS2I_OK;
}

int ds2i_hip_pipeline_wait(ds2i_hip_pipeline* p, uint64_t ticket, uint64_t* out_count, float* out_topk, uint32_t* out_topk_len,
                           ds2i_hip_stats* stats) {
    return ds2i_hip_pipeline_wait_docs(p, ticket, out_count, out_topk, nullptr, out_topk_len, stats);
}

// per kernel class of the ticket collected last (hipEvent duration of the class kernel, counters when instrumented)
int ds2i_hip_pipeline_class_stats(ds2i_hip_pipeline* p, int cls, ds2i_hip_stats* out, uint32_t* nqueries) {
    if (!p || !p->last_waited) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_class_stats: no collected ticket");
    return ds2i_hip_batch_class_stats(p->last_waited, cls, out, nqueries);
}

int ds2i_hip_pipeline_class_groups(ds2i_hip_pipeline* p, int cls, ds2i_hip_group_stats* out, uint32_t capacity, uint32_t* ngroups) {
    if (!p || !p->last_waited) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_class_groups: no collected ticket");
    return ds2i_hip_batch_class_groups(p->last_waited, cls, out, capacity, ngroups);
}

int ds2i_hip_pipeline_set_instrumented(ds2i_hip_pipeline* p, int on) {
    if (!p) return ds2i_set_error(DS2I_EINVAL, "ds2i_hip_pipeline_set_instrumented: null pipeline");
    for (auto* b : p->slots) b->instrument = on != 0;
    return DS2I_OK;
}

} // extern "C"
