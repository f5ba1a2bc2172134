// The planner of a query batch: the host part of queries.hpp (term normalisation, BM25 query weights, list ordering: queries.hpp:29-33,
// 53-56, 136-150, 357-360), the route (which kernel families answer the batch), the work units, the launch groups, the byte layout of
// the upload, result and scratch blocks, and the packed upload block itself. Plain C++: nothing here includes a HIP header or names a
// HIP type, so a stand-alone program can plan batches over an index that was never uploaded (tests/batch_plan_check.cpp). The slot that
// uploads and launches a plan is capi_batch.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#ifndef __host__ // (a plain host compiler: abi_structs.hpp marks what the kernels call too)
#define __host__
#define __device__
#endif

#include "../../include/ds2i_hip.h"
#include "abi_structs.hpp"
#include "knobs.hpp"

// Kernel classes by number of distinct query terms: <=2, <=4, <=8, <=16 keep every list's current block in LDS
// (footprint per wave grows with the class); class 4 ("long", > 16 terms -- the reference has no limit,
// queries.hpp:35-86) keeps the per-list state in a global scratch area and runs the one-document-per-step traversal.
static const int NCLS = 5;
static const int CLS_LONG = 4;
static inline int class_of(size_t nterms) { return nterms <= 2 ? 0 : nterms <= 4 ? 1 : nterms <= 8 ? 2 : nterms <= 16 ? 3 : 4; }

// one contiguous range of a batch's queries, planned by one thread (plan_queries)
struct PlanChunk {
    uint32_t q0 = 0, q1 = 0;
    std::vector<ds2i_dev::QTerm> qterms;
    std::vector<uint32_t> qnbs;
    double total_cost[NCLS] = {};
    uint32_t long_terms = 0;
    bool over16 = false; // some query of the range has more than DS2I_HIP_MAX_TERMS distinct terms
    int rc = 0;
    const char* err = nullptr;
};

// The kernel a launch group runs (SubLaunch), chosen when the plan forms the group (form_groups): the class kernel of the
// operator (ds2i_launch_batch) or one of the stream kernels (launchers.hpp; _bigk: their TopKBig instantiations, k > 64)
enum class GroupKernel : uint8_t { cls, ranked_stream, ranked_stream_bigk, ranked_stream_mixed, and_rstream, union_stream, union_stream_bigk };

// Which kernel families answer a batch: decided once per plan (plan_route), before any query is planned, from the index (its tables
// and the knobs it was uploaded with), the operator, k and the batch's flags. Two steps that depend on the queries narrow it
// (plan_queries): a query beyond 16 terms drops bigk_union, a query that goes long drops union_stream.
struct Route {
    int base_op = 0;
    bool conj = false, ranked = false, reference = false;
    bool disj_topk = false; // wand / maxscore / ranked_or
    // k > 64 (one score per lane no longer suffices): every query takes the one-document-per-step kernel with a 16-scores-
    // per-lane heap and its enumerator state in global scratch -- slower, same results (the reference has no limit on k)
    bool bigk = false;
    // ... except ranked_and on block_optpfor with every table: k_ranked_stream is compiled with 4 / 16 scores per lane too, and those
    // instantiations also take the one-term queries -- every query of 1 .. DS2I_STREAM_NT_MAX terms stays on the pruned stream path
    bool bigk_stream = false;
    // ... and wand / maxscore / ranked_or there (k_union_stream with the same heaps; their one-term queries are answered by the ranked_and seed pass)
    bool bigk_union = false;
    uint32_t stream_nt_max = 16;
    // wand / maxscore / ranked_or: the streaming form (kernels.hip, k_union_topk) needs the range tables and the block weights;
    // queries beyond 16 terms and k > 64 keep the one-document-per-step kernel, and the whole batch keeps the windowed
    // kernel when any query does (one operator = one kernel family per batch)
    bool union_stream = false;
    bool us_ok = false; // ... and its classes <= 3 may take k_union_stream (union_stream.hip): unit records + the floor words
    // (list_stream: what a stream over ONE list needs -- its blocks through the side slots; and_stream: the other lists' bitmaps as well)
    bool list_stream = false, and_stream = false;
    bool and_rs_units = false; // and / and_freq units sized for k_ranked_stream<.., AND> (cut_units: and_unit_blocks)
    // or_freq on a block_optpfor index with the side tables: the union's size by the `or` kernels, the freqs -- which do not
    // depend on the union -- by a stream of their own after the merge (freq_stream.hip)
    bool freq_stream = false;
    // ranked_and / and: the classes below rs_classes may take k_ranked_stream for their queries of 2 .. rs_nt lists
    bool rs_ok = false;
    uint32_t rs_nt = 0, rs_classes = 0;
    bool exact = false; // ... one launch group per list count (block_mixed native) instead of one per list capacity
    bool seeded = false; // a ranked_and seed pass runs first (plan_seed, seed_request)
    // DS2I_OP_TOPK_DOCS: every kernel of the batch is the *_docs instantiation of the one chosen above (the choice itself does not
    // look at the flag), the seed pass included; the result block gains the doc-ids (o_topk_docs)
    bool docs = false;
    bool goes_long(size_t nterms) const {
        if (!bigk) return nterms > DS2I_HIP_MAX_TERMS;
        if (bigk_stream) return !(nterms >= 1 && nterms <= stream_nt_max);
        if (bigk_union) return nterms > DS2I_HIP_MAX_TERMS; // (an empty query: the empty virtual query's unit, as for k <= 64)
        return true;
    }
    bool union_rstream() const { return union_stream && us_ok; }
    // classes that get unit records (BatchArgs::urec): the classes of k_ranked_stream / k_and_rstream / k_union_stream
    int urec_classes() const { return union_stream ? (us_ok ? 4 : 0) : (rs_ok && !exact) ? (int)rs_classes : 0; }
};

// union kernels (k_disjunctive) keep their decoded blocks in dynamic LDS sized per launch: a class's units are grouped
// by the list count of their query and every group is launched with just that many list slots
struct SubLaunch { uint32_t begin, end, lists; GroupKernel kernel; };

// What planning reads of an index, and nothing else: a dozen scalars and three array pointers, filled per call from an uploaded index
// (capi_internal.hpp, ds2i_plan_index) -- or made up by a test, for an index that was never uploaded.
struct PlanIndex {
    int kind = 0, num_cus = 256;
    uint64_t size = 0, num_docs = 0;
    bool has_wand = false;
    bool has_bitmaps = false;         // dense lists carry an exact bitmap behind their range-table levels
    // what the upload built (ds2i_hip_index: d_skip, d_bmw, d_rmw, side_tables(), bound_tables(), d_skip_or_pef())
    bool skip = false, bmw = false, rmw = false, side_tables = false, bound_tables = false, skip_or_pef = false;
    const Ds2iKnobs* knobs = nullptr;
    const ds2i_dev::QTerm* term_proto = nullptr; // one per list (ds2i_hip_index::term_proto)
    const uint32_t* list_n = nullptr;            // postings per list
    const float* list_topbmw = nullptr;          // per list: its DS2I_HIP_MAX_K largest block weights, descending, padded with 0
    // collection-wide BM25 statistics of an index that holds a shard (ds2i_hip_index_set_collection_stats); unset: the query weight of
    // a term comes from its list's own length and num_docs. They enter the query weight and nothing else.
    uint64_t stats_num_docs = 0;
    const uint32_t* stats_df = nullptr;          // one per list
};

// What a caller asks for
struct PlanRequest {
    int op = 0;
    uint32_t k = 0;
    const uint32_t* terms = nullptr;
    const uint32_t* query_offsets = nullptr;
    uint32_t nq = 0;
    int want_matches = 0;
    uint32_t pool_batches = 1;    // batches the caller keeps in flight beside this one (pipeline depth): unit sizing
    // a batch whose block decodes are to be counted is planned without the list streams (k_and_stream / k_freq_stream count no
    // block decodes -- ADVICE r5)
    bool no_list_streams = false;
    // ... and at k > 64 without the k-wide stream kernels (k_ranked_stream / k_union_stream with TopKBig): a profiled run launches the class
    // kernels for stream groups, and those hold DS2I_HIP_MAX_K scores -- the queries go to k_daat_long, which counts its decodes
    bool no_bigk_streams = false;
};

// Everything plan_batch decides about one batch (vectors keep their capacity from plan to plan)
struct BatchPlan {
    int op = 0;
    uint32_t k = 0, nq = 0;
    bool want_matches = false;
    uint32_t pool_batches = 1;        // as requested (seed_request carries both on)
    bool no_bigk_streams = false;
    bool use_seed = false;            // wand / maxscore / ranked_or: a ranked_and pass over seed_terms / seed_offs runs first (seed_request)
    int rc = 0;                       // what plan_batch returned, and why
    std::string err;
    Route route;
    std::vector<ds2i_dev::QTerm> qterms;
    std::vector<uint32_t> qnbs, qoff, qnb0, scratch_u32;
    std::vector<double> qcost;
    std::vector<ds2i_dev::Unit> units;
    std::vector<uint32_t> q_unit_off, split_queries, single_queries, hist_slot, cls_units[NCLS], order[NCLS];
    std::vector<float> unit_cost;
    std::vector<PlanChunk> plan_chunks;
    std::vector<unsigned long long> match_off;
    std::vector<uint32_t> seed_terms, seed_offs;
    // wand / maxscore / ranked_or as streams (k_union_topk): the virtual queries (query, driving list) their units belong to
    std::vector<ds2i_dev::QTerm> vterms;
    std::vector<uint32_t> voff, vinfo; // vinfo: {real query, exclusion lists, float bits of the query's score bound} per virtual query
    // and / and_freq: the queries whose lists all carry their exact bitmap are answered by list streams (freq_stream.hip,
    // k_and_stream) and get no work units; sterms = one record per list that has to be read
    std::vector<ds2i_dev::StreamTerm> sterms;
    uint32_t sterm_longest = 0;
    std::vector<uint32_t> empty_queries; // k > 64: the empty queries, answered without a unit (cut_units)
    uint32_t ncls[NCLS] = {};  // units per kernel class
    uint32_t nqcls[NCLS] = {}; // queries per kernel class
    uint32_t nunits = 0, nsplit = 0, nsingle = 0, long_terms = 0;
    std::vector<SubLaunch> sub[NCLS];
    // ranked_and / wand / maxscore / ranked_or: the split queries share a 256-bucket score histogram each (kernels.hip, ScoreHist)
    bool hist = false;
    // ---- one upload block (pinned mirror h_up -> d_up), byte offsets
    size_t o_vinfo = 0;
    size_t o_qterms = 0, o_qoff = 0, o_units = 0, o_q_unit_off = 0, o_split = 0, o_single = 0, o_hslot = 0, o_order[NCLS] = {}, o_urec[4] = {}, o_qterm_q = 0, o_sterms = 0,
           o_match_off = 0, up_bytes = 0;
    // ---- one result block (d_out -> pinned mirror h_out)
    size_t o_count = 0, o_topk = 0, o_topk_len = 0, o_freq_sum = 0, o_topk_docs = 0, out_bytes = 0;
    // ---- device-only scratch: per-unit partial results of split queries + the shared floors
    size_t o_unit_count = 0, o_unit_topk = 0, o_unit_topk_len = 0, o_unit_freq_sum = 0, o_unit_topk_docs = 0, o_qfloor = 0, o_qfloorw = 0, scr_bytes = 0;
};

// validate + route, per-query planning, work units, launch groups, layout, seed terms -- in that order. Returns DS2I_OK or an error code,
// which it also leaves in plan.rc with its message in plan.err.
int plan_batch(BatchPlan& plan, const PlanIndex& ix, const PlanRequest& rq);
// the seed pass of a plan with use_seed: a ranked_and batch of its own over sub-queries of the same queries, planned like any other
PlanRequest seed_request(const BatchPlan& plan);
// the upload block of a plan, up_bytes of it, as the kernels read it
void pack_upload(const BatchPlan& plan, uint8_t* dst);
