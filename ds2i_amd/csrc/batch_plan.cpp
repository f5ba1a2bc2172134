// The planner of a query batch (batch_plan.hpp): host code only -- no HIP call, no HIP header. plan_batch turns a request into a
// BatchPlan; pack_upload writes the plan's upload block. The host plans batch i+1 while the kernels of batch i run (capi_batch.cpp).
#include <algorithm>
#include <atomic>
#include <exception>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <limits>
#include <new>
#include <pthread.h>

#include "batch_plan.hpp"
#include "host_index.hpp"
#include "unit_cut.hpp"

using ds2i_dev::QTerm;
using ds2i_dev::Unit;

// fn(0) .. fn(n-1), fn(0) on the calling thread and the others on a small pool of planning threads that lives as long as the
// library (created on first use; a batch is planned ~200 times a second, so the threads are kept, not spawned per batch)
namespace {
struct PlanPool {
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::vector<std::thread> threads;
    const std::function<void(unsigned)>* fn = nullptr;
    unsigned next = 0, total = 0, done = 0;
    uint64_t epoch = 0;
    std::exception_ptr failed; // the first exception a piece threw (any thread); rethrown by run() once every piece is done
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv_work.wait(lk, [&] { return epoch != seen && next < total; });
            while (next < total) {
                const unsigned i = next++;
                const std::function<void(unsigned)>* f = fn;
                lk.unlock();
                std::exception_ptr ex;
                try { (*f)(i); } catch (...) { ex = std::current_exception(); } // (a throw on a detached thread would be std::terminate)
                lk.lock();
                if (ex && !failed) failed = ex;
                if (++done == total) cv_done.notify_all();
            }
            seen = epoch;
        }
    }
    void run(unsigned n, const std::function<void(unsigned)>& f) {
        if (n <= 1) { if (n) f(0); return; }
        {
            std::lock_guard<std::mutex> lk(mu);
            while (threads.size() + 1 < n) { threads.emplace_back([this] { worker(); }); threads.back().detach(); }
            fn = &f;
            next = 1; // (index 0 is the caller's)
            total = n;
            done = 1;
            failed = nullptr;
            ++epoch;
        }
        cv_work.notify_all();
        std::exception_ptr ex;
        try { f(0); } catch (...) { ex = std::current_exception(); }
        // whatever happened to piece 0, the workers hold a pointer to f and to the caller's chunks: they are waited for
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return done == total; });
        total = 0;
        fn = nullptr;
        if (!ex) ex = failed;
        failed = nullptr;
        lk.unlock();
        if (ex) std::rethrow_exception(ex);
    }
};
std::mutex g_plan_pool_user; // one batch at a time uses the pool (several pipelines / replicas may plan concurrently)
std::atomic<PlanPool*> g_plan_pool{nullptr};
// fork(): the child has the parent's PlanPool bookkeeping (threads.size() > 0, perhaps a batch half planned, perhaps the user
// mutex held by a thread that does not exist there) and none of its threads -- it starts over with an empty pool and a fresh mutex
void plan_pool_after_fork_in_child() {
    g_plan_pool.store(new PlanPool, std::memory_order_release); // (the old one is leaked: its mutex may be held)
    new (&g_plan_pool_user) std::mutex;
}
void ds2i_plan_pool_run(unsigned n, const std::function<void(unsigned)>& f) {
    static const bool once = [] {
        g_plan_pool.store(new PlanPool, std::memory_order_release); // (leaked on purpose: its detached threads may outlive static destruction)
        pthread_atfork(nullptr, nullptr, plan_pool_after_fork_in_child);
        return true;
    }();
    (void)once;
    PlanPool* const pool = g_plan_pool.load(std::memory_order_acquire);
    if (n > 1 && g_plan_pool_user.try_lock()) {
        std::lock_guard<std::mutex> user(g_plan_pool_user, std::adopt_lock); // (released when run() throws, too)
        pool->run(n, f);
    } else {
        for (unsigned i = 0; i < n; ++i) f(i); // the pool is busy with another batch: plan this one on the caller's thread
    }
}
} // namespace

namespace {

inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

// the error a plan ends with (BatchPlan::rc / err): capi_batch.cpp hands both to ds2i_set_error
int fail(BatchPlan& b, int rc, const char* msg) {
    b.rc = rc;
    b.err = msg;
    return rc;
}

// units in decreasing cost order. The order only steers the dispatcher (big units first, small ones fill the tail), so
// a counting sort on the float's exponent and top mantissa bits replaces the comparison sort: O(n), stable.
void order_by_cost(const std::vector<float>& cost, const std::vector<uint32_t>& ids, std::vector<uint32_t>& out,
                   std::vector<uint32_t>& tmp) {
    const int BITS = 14; // 8 exponent bits + 6 mantissa bits of a positive float
    const size_t NB = size_t(1) << BITS;
    tmp.assign(NB + 1, 0);
    auto key = [&](uint32_t id) -> uint32_t {
        uint32_t bits;
        const float c = cost[id] > 0.f ? cost[id] : 0.f;
        std::memcpy(&bits, &c, 4);
        return (uint32_t)(NB - 1) - (bits >> (31 - BITS)); // descending
    };
    for (uint32_t id : ids) ++tmp[key(id) + 1];
    for (size_t i = 0; i < NB; ++i) tmp[i + 1] += tmp[i];
    out.resize(ids.size());
    for (uint32_t id : ids) out[tmp[key(id)]++] = id;
}

// ---------------------------------------------------------------- plan: host half of the query operators
// validate + route, per-query planning, work units, launch groups, layout, seed terms -- in that order (plan_batch, at the end)

// the operator and k checked, the batch's header set, b.route decided
static int plan_route(BatchPlan& b, const PlanIndex& ix, const PlanRequest& rq) {
    const Ds2iKnobs& kn = *ix.knobs;
    const int op = rq.op;
    uint32_t k = rq.k;
    const int base_op = op & 0xFF;
    if (base_op < DS2I_OP_AND || base_op > DS2I_OP_RANKED_OR || (op & ~(0xFF | DS2I_OP_REFERENCE_ORDER | DS2I_OP_NO_COUNTERS | DS2I_OP_TOPK_DOCS)))
        return fail(b, DS2I_EINVAL, "ds2i_hip_batch_prepare: unknown query operator");
    if ((op & DS2I_OP_TOPK_DOCS) && base_op < DS2I_OP_RANKED_AND)
        return fail(b, DS2I_EINVAL, "DS2I_OP_TOPK_DOCS: and / and_freq / or / or_freq return no top-k");
    Route r;
    r.docs = (op & DS2I_OP_TOPK_DOCS) != 0;
    r.base_op = base_op;
    r.conj = base_op == DS2I_OP_AND || base_op == DS2I_OP_AND_FREQ || base_op == DS2I_OP_RANKED_AND;
    r.ranked = base_op >= DS2I_OP_RANKED_AND;
    r.reference = (op & DS2I_OP_REFERENCE_ORDER) != 0;
    if (r.ranked && !ix.has_wand) return fail(b, DS2I_ENOWAND, "ranked operator needs wand data");
    if (r.ranked && (k == 0 || k > DS2I_HIP_MAX_K_LONG)) return fail(b, DS2I_EINVAL, "k must be in [1, DS2I_HIP_MAX_K_LONG]");
    if (!r.ranked) k = 1; // and / or return counts only: k is ignored, no top-k is produced or copied
    b.op = op;
    b.k = k;
    b.nq = rq.nq;
    b.want_matches = rq.want_matches && (base_op == DS2I_OP_AND || base_op == DS2I_OP_AND_FREQ);
    b.pool_batches = rq.pool_batches;
    b.no_bigk_streams = rq.no_bigk_streams;

    const bool and_op = base_op == DS2I_OP_AND || base_op == DS2I_OP_AND_FREQ;
    const bool disj_topk = r.disj_topk = base_op == DS2I_OP_WAND || base_op == DS2I_OP_MAXSCORE || base_op == DS2I_OP_RANKED_OR;
    const bool stream_tables = ix.side_tables && ix.bound_tables; // what k_ranked_stream and k_union_stream read
    r.bigk = r.ranked && k > DS2I_HIP_MAX_K;
    const bool bigk_ok = r.bigk && !rq.no_bigk_streams && !r.reference && stream_tables && !kn.no_ranked_stream && kn.stream_nt_max >= 4;
    r.bigk_stream = bigk_ok && base_op == DS2I_OP_RANKED_AND;
    r.bigk_union = bigk_ok && disj_topk && !kn.no_union_rstream;
    r.stream_nt_max = kn.stream_nt_max;
    // ranked_or takes the seed only in its block-synchronous form: its reference-order traversal stays the unpruned
    // exhaustive OR of queries.hpp:404-476 (the oracle the reference tests wand / maxscore against)
    r.seeded = (!r.bigk || r.bigk_union) && (base_op == DS2I_OP_WAND || base_op == DS2I_OP_MAXSCORE || (base_op == DS2I_OP_RANKED_OR && !r.reference));
    // (any codec: k_union_topk walks the driving list by its skip table or chunk directory; k_union_stream also decodes through the side tables)
    r.union_stream = disj_topk && !r.reference && (!r.bigk || r.bigk_union) && ix.bound_tables && ix.skip_or_pef;
    r.us_ok = !kn.no_union_rstream && stream_tables;
    r.list_stream = and_op && !r.reference && !b.want_matches && ix.side_tables && !kn.no_list_streams && !rq.no_list_streams;
    r.and_stream = r.list_stream && ix.rmw && ix.has_bitmaps;
    r.and_rs_units = and_op && !r.reference && stream_tables && !kn.no_ranked_stream;
    r.freq_stream = base_op == DS2I_OP_OR_FREQ && !r.reference && ix.side_tables && !kn.no_list_streams && !rq.no_list_streams;
    // ranked_and on block_optpfor with every upload-time table: the 2- .. 8-term queries (block_mixed native: 2 .. 4) run the pipelined stream
    // kernel compiled for exactly their list count (ranked_stream.hip), one launch group per count, back to back on the
    // class stream; one-term queries and everything else keep the class kernel
    // (the 5..8-term class takes the stream kernel too, up to DS2I_STREAM_NT_MAX lists -- block_optpfor only)
    // `and` batches that do not ask for the doc-id lists take the same pipeline with AND = true -- a candidate whose hints settle
    // its membership in every other list is counted without any of them being searched or decoded (k_conjunctive<false, ...>
    // verifies every survivor of its filters by a probe).
    const bool rs_and = and_op && ix.kind == DS2I_BLOCK_OPTPFOR; // (with or without the doc-id lists)
    // k_ranked_stream is compiled for the list capacities 2 | 4 | 6 | 8; the planner hands it the queries of 2 .. DS2I_STREAM_NT_MAX lists
    // (default 8; 4 = the 5..8-term class keeps k_conjunctive<.., 8>). Round 5, interleaved on one box: 1 047-1 060 k queries/s with 8
    // against 985-992 k with 4.
    r.rs_nt = ix.kind == DS2I_BLOCK_OPTPFOR ? kn.stream_nt_max : 4u;
    r.rs_classes = r.rs_nt > 8 ? 4u : r.rs_nt > 4 ? 3u : 2u;
    r.exact = ix.kind != DS2I_BLOCK_OPTPFOR;
    // (block_mixed native has no side slots: k_ranked_stream_mixed parses its blocks by type byte, over the skip table)
    r.rs_ok = (base_op == DS2I_OP_RANKED_AND || rs_and) && !r.reference && (!r.bigk || r.bigk_stream) && !kn.no_ranked_stream &&
              (ix.side_tables || (ix.kind == DS2I_BLOCK_MIXED && ix.skip)) && ix.bound_tables;
    b.route = r;
    return DS2I_OK;
}

// The per-query half of planning for the queries [ch.q0, ch.q1) (normalisation, BM25 query weights, list order, costs, bounds): the
// terms into the chunk's own vectors, the per-query values into the batch's arrays at those queries (plan_queries)
static void plan_range(BatchPlan& b, const PlanIndex& ix, const uint32_t* terms, const uint32_t* query_offsets, PlanChunk& ch) {
    const Route& r = b.route;
    const bool conj = r.conj, ranked = r.ranked, bigk = r.bigk;
    const uint32_t k = b.k;
    std::vector<QTerm>& qterms = ch.qterms;
    std::vector<uint32_t>& qnbs = ch.qnbs;
    std::vector<uint32_t>& qnb0 = b.qnb0;
    std::vector<uint32_t> t;
    std::vector<std::pair<uint32_t, uint32_t>> tf; // (term, query term frequency)
    qterms.clear();
    qnbs.clear();
    for (uint32_t q = ch.q0; q < ch.q1; ++q) {
        if (query_offsets[q + 1] < query_offsets[q])
            { ch.rc = DS2I_EINVAL; ch.err = "query_offsets must be non-decreasing"; return; }
        t.assign(terms + query_offsets[q], terms + query_offsets[q + 1]);
        std::sort(t.begin(), t.end()); // queries.hpp:31 / 139
        tf.clear();
        for (size_t i = 0; i < t.size(); ++i) {
            if (t[i] >= ix.size) { ch.rc = DS2I_ETERM; ch.err = "term id out of range"; return; }
            if (i == 0 || t[i] != t[i - 1]) tf.emplace_back(t[i], 1u);
            else tf.back().second += 1;
        }
        if (tf.size() > DS2I_HIP_MAX_TERMS_LONG)
            { ch.rc = DS2I_ETOOLONG; ch.err = "query has more than DS2I_HIP_MAX_TERMS_LONG distinct terms"; return; }
        const size_t begin = qterms.size();
        for (auto const& p : tf) {
            QTerm qt = ix.term_proto[p.first]; // one cache line: see capi_internal.hpp
            const float mtw = qt.q_weight, lbmw = qt.max_weight;
            const uint32_t nb = qt.nblocks;
            qt.q_weight = qt.max_weight = 0.f;
            if (ranked) {
                qt.q_weight = ix.stats_df ? ds2i_host::bm25::query_term_weight(p.second, ix.stats_df[p.first], ix.stats_num_docs)
                                          : ds2i_host::bm25::query_term_weight(p.second, qt.n, ix.num_docs);
                qt.max_weight = qt.q_weight * mtw;
                qt.max_bmw = ix.bmw ? qt.q_weight * lbmw : std::numeric_limits<float>::infinity();
                qt.rmw_scale = qt.q_weight * (lbmw * (1.0f / 255.0f)); // range-table byte -> bound of the term score
            }
            qterms.push_back(qt);
            qnbs.push_back(nb);
        }
        double cost = 0;
        if (conj) { // sort by increasing frequency (queries.hpp:53-56, 357-360); stable insertion sort of <= a few lists
            for (size_t i = begin + 1; i < qterms.size(); ++i) {
                const QTerm v = qterms[i];
                const uint32_t vn = qnbs[i];
                size_t j = i;
                while (j > begin && v.n < qterms[j - 1].n) {
                    qterms[j] = qterms[j - 1];
                    qnbs[j] = qnbs[j - 1];
                    --j;
                }
                qterms[j] = v;
                qnbs[j] = vn;
            }
            if (!tf.empty()) {
                const double n0 = qterms[begin].n;
                qnb0[q] = qnbs[begin];
                cost = qnb0[q] * (ranked ? 2.0 : 1.0);
                for (size_t i = begin + 1; i < qterms.size(); ++i) cost += std::min<double>(qnbs[i], n0);
                // With range tables (BatchArgs::rmw) a ranked conjunction is a walk over the blocks of its shortest list --
                // most of them are left after one decode and one gather per other list -- so a unit's time goes with its
                // number of list-0 blocks, a little more per block the more lists there are (measured wave time per round:
                // 6 / 10 / 15 us for the <=2- / <=4- / <=8-list classes)
                if (ranked && ix.rmw && tf.size() > 1) {
                    cost = qnb0[q] * (3.0 + (double)tf.size());
                    // ... unless the bounds have little to work with. A block of the driving list is cheap when the heap threshold
                    // kills its candidates at the range tables; how many instead get as far as a lookup in the other lists goes with
                    // (a) how many sit in an occupied range of every other list (~1/4 per list: the tables hold 4-8 entries per
                    // posting) and (b) how high the threshold can be -- the k-th best of an expected M = n0 * prod(n_j / N) matches:
                    // with M in the hundreds a few candidates of every block pass, with M in the 100 000s none. A lookup costs a
                    // block search + a decode of another list's block, about 4x the block's own cost (measured: 9 us per block for
                    // two 80 k-posting lists against 2 us for the typical unit; left unsplit such queries were the kernel's tail).
                    double M = (double)qterms[begin].n, inrange = 128.0;
                    for (size_t i = begin + 1; i < qterms.size(); ++i) {
                        M *= (double)qterms[i].n / (double)ix.num_docs;
                        inrange *= 0.25;
                    }
                    const double span_entries = 128.0 * (double)ix.num_docs / std::max(1.0, (double)qterms[begin].n) /
                                                (double)(1u << std::min(31u, qterms[begin + 1].rmw_shift));
                    const double lookups = inrange * std::min(1.0, 3.0 * (double)k / std::max(1.0, M)) * std::min(1.0, span_entries / 128.0);
                    cost *= 1.0 + 3.5 * std::min(1.0, lookups);
                }
                // a one-term ranked query scans its block weights (64 per probe) and decodes about k blocks
                if (ranked && ix.bmw && tf.size() == 1) cost = qnb0[q] / 16.0 + 4.0 * k;
                b.match_off[q + 1] = 128ull * qnb0[q];
            }
        } else {
            for (size_t i = begin; i < qterms.size(); ++i) cost += qnbs[i] * (ranked ? 2.0 : 1.0);
        }
        if (ranked && ix.bmw && qterms.size() > begin) {
            // ranked_and pruning bounds (kernels.hip): suffix sums of the list bounds in enumerator order; a one-term
            // query additionally starts from the k-th largest block weight of its list
            float suf = 0.f;
            for (size_t i = qterms.size(); i-- > begin;) {
                qterms[i].suf_bmw = suf;
                suf += qterms[i].max_bmw;
            }
            // (list_topbmw holds DS2I_HIP_MAX_K entries per list; the k > 64 path does not use static floors)
            if (!bigk && qterms.size() - begin == 1)
                qterms[begin].floor1 = qterms[begin].q_weight * ix.list_topbmw[(size_t)tf[0].first * DS2I_HIP_MAX_K + (k - 1)];
            if (!bigk && !conj) { // top-k of the UNION: any one term's k-th best block weight is a floor of the k-th score
                float f = 0.f;
                for (size_t i = 0; i < tf.size(); ++i)
                    f = std::max(f, qterms[begin + i].q_weight * ix.list_topbmw[(size_t)tf[i].first * DS2I_HIP_MAX_K + (k - 1)]);
                qterms[begin].floor1 = f;
            }
        }
        b.qoff[q + 1] = (uint32_t)(qterms.size() - begin); // (terms of this query: turned into offsets once the ranges are joined)
        b.qcost[q] = cost;
        ch.total_cost[r.goes_long(tf.size()) ? CLS_LONG : class_of(tf.size())] += cost;
        if (tf.size() > DS2I_HIP_MAX_TERMS) ch.over16 = true;
        if (r.goes_long(tf.size())) ch.long_terms = std::max<uint32_t>(ch.long_terms, (uint32_t)std::max<size_t>(1, tf.size()));
    }
}

// The per-query half of planning (normalisation, BM25 query weights, list order, costs, bounds) is independent from query
// to query: the batch is cut into contiguous ranges, one per planning thread (DS2I_PLAN_THREADS, default 4, the caller's
// thread takes the first range), each range fills vectors of its own, and the ranges are joined by one copy. At
// configs[1] scale the host's 0.9 ms of planning per 1.3 ms of kernels is what bounds the end-to-end rate, and the
// same holds for a batch cut over 8 GPUs; the unit list and the class orders below stay sequential.
// all_cost: the cost of the whole batch (cut_units sizes its units by it)
static int plan_queries(BatchPlan& b, const PlanIndex& ix, const uint32_t* terms, const uint32_t* query_offsets, double& all_cost) {
    Route& r = b.route;
    const uint32_t nq = b.nq;
    b.qoff.assign(nq + 1, 0);
    b.qcost.assign(nq, 0.0);
    b.qnb0.assign(nq, 0);
    b.match_off.assign(nq + 1, 0);
    b.long_terms = 0;
    // default: 4, but never more than this process's share of the CPUs it may use -- one rank per GPU under torchrun
    // (LOCAL_WORLD_SIZE) on a host whose cgroup grants 16 CPUs leaves each of 8 ranks one planning thread
    static const unsigned default_threads = [] {
        double cpus = (double)std::max(1u, std::thread::hardware_concurrency());
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) { // cgroup v2: "<quota> <period>" or "max <period>"
            char q[32] = {0};
            double per = 0;
            if (std::fscanf(f, "%31s %lf", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0) cpus = std::min(cpus, std::atof(q) / per);
            std::fclose(f);
        }
        const char* lw = std::getenv("LOCAL_WORLD_SIZE");
        const double ranks = lw && std::atoi(lw) > 0 ? (double)std::atoi(lw) : 1.0;
        const double mine = cpus / ranks - 1.0; // (one for the thread that drives the pipeline)
        return (unsigned)std::max(1.0, std::min(4.0, mine));
    }();
    const unsigned want_threads = ix.knobs->plan_threads ? ix.knobs->plan_threads : default_threads;
    const unsigned nchunks = nq >= 1024 ? std::max(1u, std::min(want_threads, 16u)) : 1u;
    std::vector<PlanChunk>& chunks = b.plan_chunks;
    if (chunks.size() < nchunks) chunks.resize(nchunks);
    for (unsigned c = 0; c < nchunks; ++c) {
        chunks[c].q0 = (uint32_t)((uint64_t)nq * c / nchunks);
        chunks[c].q1 = (uint32_t)((uint64_t)nq * (c + 1) / nchunks);
        chunks[c].rc = 0;
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        for (unsigned c = 0; c < nchunks; ++c) {
            chunks[c].long_terms = 0;
            chunks[c].over16 = false;
            for (double& v : chunks[c].total_cost) v = 0;
        }
        ds2i_plan_pool_run(nchunks, [&](unsigned c) { plan_range(b, ix, terms, query_offsets, chunks[c]); });
        for (unsigned c = 0; c < nchunks; ++c)
            if (chunks[c].rc) return fail(b, chunks[c].rc, chunks[c].err);
        // k > 64 through the union streams needs the whole batch on them (the kernels see virtual queries; k_daat_long does not): a
        // query beyond 16 terms sends the batch back to the one-document-per-step kernels -- planned again, once
        bool over = false;
        for (unsigned c = 0; c < nchunks; ++c) over = over || chunks[c].over16;
        if (!(r.bigk_union && over)) break;
        r.bigk_union = false;
        r.union_stream = r.seeded = false; // (at k > 64 both came with bigk_union: plan_route)
    }
    size_t total = 0;
    for (unsigned c = 0; c < nchunks; ++c) total += chunks[c].qterms.size();
    b.qterms.resize(total);
    b.qnbs.resize(total);
    size_t at = 0;
    double total_cost[NCLS] = {};
    for (unsigned c = 0; c < nchunks; ++c) {
        if (!chunks[c].qterms.empty()) {
            std::memcpy(b.qterms.data() + at, chunks[c].qterms.data(), chunks[c].qterms.size() * sizeof(QTerm));
            std::memcpy(b.qnbs.data() + at, chunks[c].qnbs.data(), chunks[c].qnbs.size() * 4);
        }
        at += chunks[c].qterms.size();
        for (int k2 = 0; k2 < NCLS; ++k2) total_cost[k2] += chunks[c].total_cost[k2];
        b.long_terms = std::max(b.long_terms, chunks[c].long_terms);
    }
    for (uint32_t q = 0; q < nq; ++q) b.qoff[q + 1] += b.qoff[q];
    for (uint32_t q = 0; q < nq; ++q) b.match_off[q + 1] += b.match_off[q];
    if (b.long_terms) r.union_stream = false; // (a query goes long: the whole batch keeps the windowed kernel -- Route::union_stream)
    all_cost = 0;
    for (double c : total_cost) all_cost += c;
    return DS2I_OK;
}

void add_unit(BatchPlan& b, int c, uint32_t q, uint32_t lo, uint32_t hi, uint32_t parts, double cost) {
    b.cls_units[c].push_back((uint32_t)b.units.size());
    b.units.push_back(Unit{q, lo, hi, parts});
    b.unit_cost.push_back((float)cost);
}

// and / and_freq of a query whose lists all carry their exact bitmap (cut_units): the query is a sum over the postings of its shortest
// list (and, with the freqs, over every list's own postings) of one bit test per other list -- list streams, no units (k_and_stream)
// (and_query reads only its shortest list: that one needs no bitmap of its own)
// One-term queries (and_query walks the list and counts it, queries.hpp:58-84): the same stream with no other list -- beside
// the class kernels instead of in front of the two-term group on class 0's stream (424 of 4096 queries, 5 of that class's 9 ms)
// Returns false, and adds nothing, when a list lacks its bitmap.
bool add_list_streams(BatchPlan& b, const PlanIndex& ix, uint32_t q, uint32_t nt) {
    const int base_op = b.route.base_op;
    const std::vector<QTerm>& qterms = b.qterms;
    const std::vector<uint32_t>& qoff = b.qoff;
    bool dense = true;
    for (uint32_t i = qoff[q] + (base_op == DS2I_OP_AND ? 1u : 0u); nt > 1 && i < qoff[q + 1]; ++i)
        dense = dense && ds2i_dev::RmwLevels::has_bitmap(qterms[i].n, (uint32_t)ix.num_docs);
    if (!dense) return false;
    const uint32_t lists = base_op == DS2I_OP_AND_FREQ ? nt : 1u;
    for (uint32_t i = 0; i < lists; ++i) {
        const QTerm& t = qterms[qoff[q] + i];
        ds2i_dev::StreamTerm st{};
        st.list_off = t.list_off;
        st.tail = t.aux1;
        st.n = t.n;
        st.blk_base = t.blk_base;
        st.q = q;
        st.counts = i == 0 ? 1u : 0u;
        st.nother = nt - 1;
        uint32_t k2 = 0;
        for (uint32_t j = 0; j < nt; ++j) {
            if (j == i) continue;
            const QTerm& o = qterms[qoff[q] + j];
            st.bm[k2++] = 64ull * o.rmw_off64 + ds2i_dev::RmwLevels((uint32_t)ix.num_docs, o.rmw_shift).bytes();
        }
        b.sterms.push_back(st);
        b.sterm_longest = std::max(b.sterm_longest, t.nblocks);
    }
    return true;
}

// wand / maxscore / ranked_or as streams (cut_units): the virtual queries of query q (one per driving list) and their units
void cut_union_query(BatchPlan& b, uint32_t q, int c, uint32_t ut_blocks) {
    const std::vector<QTerm>& qterms = b.qterms;
    const uint32_t nt = b.qoff[q + 1] - b.qoff[q];
    // lists by decreasing max score (device-computed list maxima x query weight); a document belongs to the first
    // list of that order that holds it, so what list e owns scores at most S_e = the maxima from e down. A list
    // whose S_e is below the static floor (some term's k-th best block weight) gets no units at all -- MaxScore's
    // non-essential lists, decided at plan time; the kernel re-checks against the live threshold.
    const size_t begin = b.qoff[q];
    uint32_t ord[DS2I_HIP_MAX_TERMS];
    for (uint32_t i = 0; i < nt; ++i) ord[i] = i;
    for (uint32_t i = 1; i < nt; ++i) { // stable insertion sort, descending max score
        const uint32_t v = ord[i];
        uint32_t j = i;
        while (j > 0 && qterms[begin + v].max_bmw > qterms[begin + ord[j - 1]].max_bmw) { ord[j] = ord[j - 1]; --j; }
        ord[j] = v;
    }
    float suffix[DS2I_HIP_MAX_TERMS + 1];
    suffix[nt] = 0.f;
    for (uint32_t e = nt; e-- > 0;) suffix[e] = suffix[e + 1] + qterms[begin + ord[e]].max_bmw;
    const float f1 = qterms[begin].floor1;
    const size_t first_unit = b.units.size();
    for (uint32_t e = 0; e < nt; ++e) {
        if (e && suffix[e] * (1.0f + 1.0f / 65536.0f) < f1 * (1.0f - 1.0e-5f)) break; // this list and all after it: non-essential
        const uint32_t vq = (uint32_t)b.voff.size() - 1;
        QTerm drv = qterms[begin + ord[e]];
        drv.suf_bmw = suffix[e + 1];
        drv.floor1 = f1;
        drv.max_weight = suffix[0]; // (k_union_stream: the query's score bound = the scale of its shared histogram)
        b.vterms.push_back(drv);
        for (uint32_t j = 0; j < e; ++j) { // exclusion lists
            QTerm t = qterms[begin + ord[j]];
            t.suf_bmw = suffix[e + 1];
            b.vterms.push_back(t);
        }
        for (uint32_t j = e + 1; j < nt; ++j) { // optional lists
            QTerm t = qterms[begin + ord[j]];
            t.suf_bmw = suffix[j + 1];
            b.vterms.push_back(t);
        }
        b.voff.push_back((uint32_t)b.vterms.size());
        uint32_t sbits;
        std::memcpy(&sbits, &suffix[0], 4);
        b.vinfo.push_back(q);
        b.vinfo.push_back(e);
        b.vinfo.push_back(sbits);
        const uint32_t nbe = std::max(1u, b.qnbs[begin + ord[e]]);
        // (the 9-16-term class runs two waves per SIMD: its units are cut 4 times finer, for more of them at once)
        const uint32_t utb_c = c == 3 ? std::max(4u, ut_blocks / 4u) : ut_blocks;
        const uint32_t parts_e = (nbe + utb_c - 1) / utb_c, per = (nbe + parts_e - 1) / parts_e;
        for (uint32_t lo = 0; lo < nbe; lo += per) // (the driving lists of higher max score first: they raise the threshold)
            add_unit(b, c, vq, lo, std::min(nbe, lo + per), 0, (double)(nt - e) * 1.0e7 + (double)(std::min(nbe, lo + per) - lo));
    }
    const uint32_t total = (uint32_t)(b.units.size() - first_unit);
    for (size_t ui = first_unit; ui < b.units.size(); ++ui) b.units[ui].nparts = total;
    if (total > 1) b.split_queries.push_back(q);
}

// Ranked conjunctions with range tables, batches of 1536 queries and more (cut_units): the parts of a split query taper (unit_cut.hpp) --
// the first one (1 - taper_ratio) of the query but at most taper_cap equal parts, each next one taper_ratio times the one before, down
// to the equal part; a part costs its share of the blocks, so that the class order (costliest first) starts a query's large parts first.
// cap_blocks (DS2I_UNIT_CAP; 0 = none) bounds every part, the first included. Measured on the GOV2-scale batch, 4096 queries, one
// index, four interleaved rounds of 60 pipelined steps each (median queries/s, units per batch without the two-list stream group,
// which the listing left out): equal cut 1 071 k, 50.1 k units | ratio 1/2, cap 2: 1 122 k, 48.0 k | 1/2, 4: 1 059 k, 43.2 k |
// 1/2, 8: 721 k, 35.5 k | 2/3, 2: 1 134 k, 48.2 k | 2/3, 4: 1 049 k, 42.6 k | 2/3, 8: 790 k, 34.1 k; the spread of a point over its
// rounds is 1-8 k except 2/3, 4 (17 k). A first part of 4 or 8 equal parts becomes the tail of its launch group.
static void add_tapering_units(BatchPlan& b, int c, uint32_t q, uint32_t nb0, uint32_t parts, uint32_t cap_blocks, double cost,
                               std::vector<uint32_t>& cut) {
    const double taper_ratio = 2.0 / 3.0, taper_cap = 2.0;
    parts = ds2i_cut::cut_blocks(nb0, parts, taper_ratio, taper_cap, cap_blocks, cut);
    if (parts > 1) b.split_queries.push_back(q);
    for (uint32_t j = 0; j < parts; ++j) add_unit(b, c, q, cut[j], cut[j + 1], parts, ds2i_cut::part_cost(cost, nb0, cut[j], cut[j + 1]));
}
// What starting a unit costs, in the cost model's units: where the parts taper, a part's own work is never priced below it. Measured on
// the GOV2-scale batch: 62.6 M units of cost run for 17.9 s of wave time (DS2I_UNIT_CLOCK, the sum of the unit times), 0.29 us per unit
// of cost; unit setup is 0.8 % of a two-list unit's cycles (median unit 650 us: 5 us) and 8 % / 24 % of a three- / four-list unit's
// (mean unit 208 us, setup 15 % of the two together: 30 us). The 256 floor is above both; beyond 8 lists (floor 48) nothing was
// measured, and the four-list figure is taken -- at 1536 queries and more that class's target is above it as well.
static double unit_start_cost(uint32_t nt) { return nt <= 2 ? 17.0 : 105.0; }

// ---- work units: long conjunctive queries are split by block ranges of their shortest list so
// that one giant query does not pin a single wavefront (SURVEY.md §7 "Load imbalance")
// all_cost: the batch's cost (plan_queries), scaled here to the batches in flight
static void cut_units(BatchPlan& b, const PlanIndex& ix, double& all_cost) {
    const Route& r = b.route;
    const uint32_t nq = b.nq;
    const std::vector<uint32_t>& qoff = b.qoff;
    const std::vector<uint32_t>& qnb0 = b.qnb0;
    const std::vector<double>& qcost = b.qcost;
    b.units.clear();
    b.unit_cost.clear();
    b.q_unit_off.assign(nq + 1, 0);
    b.split_queries.clear();
    b.single_queries.clear();
    b.empty_queries.clear();
    for (int c = 0; c < NCLS; ++c) {
        b.cls_units[c].clear();
        b.nqcls[c] = 0;
    }
    b.sterms.clear();
    b.sterm_longest = 0;
    b.vterms.clear();
    b.voff.assign(1, 0);
    b.vinfo.clear();
    // A pipeline keeps several batches in flight: a small batch shares the wave slots with its neighbours, so its units are sized as if
    // two or three of them were one batch. Sized against its own cost alone a 512-query batch was cut into 20 k units -- three and a half
    // full rounds of the wave slots, each unit paying its window fill and its heap's warm-up. Measured at GOV2 scale (queries/s with the
    // multiplier 1 | 1.5 | 2 | 3 | depth): 256 queries 305 k | 349 k | 376 k | 414 k | 359 k; 512: 438 k | 474 k | 522 k | 552 k | 343 k;
    // 1024: 695 k | 784 k | 844 k | 687 k | 591 k; 2048 (two in 4096): 780 k | 944 k | 990 k.
    all_cost *= std::min<double>(std::min<double>(nq <= 512 ? 3.0 : 2.0, std::max<uint32_t>(1u, b.pool_batches)), std::max(1.0, 4096.0 / std::max(1u, nq)));
    const double resident = ix.num_cus * 24.0; // waves the concurrent kernels share
    // units per resident wave (tuning knob, DS2I_UNIT_FACTOR): more = better tail balance, more per-unit overhead
    // With range tables a ranked conjunction is cheap per block and the parts of a split query each pay for warming up
    // their own heap: coarser units win (measured on the GOV2-scale batch with the block-synchronous kernels of round 3, queries/s:
    // factor 16: 355 k, 8: 344 k, 4 with the many-list classes cut 4x finer: 430-457 k, 2: 251 k; with the stream kernels and the tapering cut below, 4096 queries:
    // factor 2: 930 k, 4: 1 119-1 136 k over four runs, 8: 1 146 k in its one run -- no worse than 4, not told apart from it)
    const bool rmw_units = r.ranked && r.conj && ix.rmw; // (and / and_freq verify every candidate the tables let through: their cost
                                                             // stays with the blocks of all lists, and they are throughput-, not tail-bound: measured)
    // (a small batch -- the per-GPU share of a batch sharded over several GPUs -- is cut coarser still: at 512 queries factor 2
    // measured 391 k queries/s against 321-328 k with 4; at 4096 it is the other way round)
    const double unit_factor = ix.knobs->unit_factor > 0 ? ix.knobs->unit_factor : rmw_units ? (nq < 1536 ? 2.0 : 4.0) : 16.0;
    const uint32_t and_unit_blocks = 96u; // (measured, `and`: 48: 965 k, 96: 1 068 k, 192: 1 190 k against 1 360 k of the same build, whole queries: 802 k; and_freq: 24 | 48 | 96 all 334-337 k)
    const uint32_t ut_blocks = ix.knobs->ut_blocks; // DS2I_UT_BLOCKS, default 320: blocks of the driving list per unit (k_union_topk, round 4: 96: 335 k, 128-256: 345-352 k, 384: 335 k queries/s; k_union_stream, round 6: 64: 240 k, 160: 378 k, 320: 401 k)
    const bool split_ok = r.conj && !r.reference;
    // (ranked conjunctions with range tables, batches of 1536 queries and more: the parts of a split query taper -- add_tapering_units)
    const bool taper_batch = rmw_units && split_ok && nq >= 1536;
    std::vector<uint32_t> cut;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t nt = qoff[q + 1] - qoff[q];
        const int c = r.goes_long(nt) ? CLS_LONG : class_of(nt);
        // multi-list units are latency-bound chains (non-sequential probes): cut 4x finer so the tail stays parallel; the 9-16-term
        // class (one or two waves per SIMD; its few, long units were the last thing every batch waited for) 4x finer still
        const bool rmw_cost = rmw_units; // (cost already counts the class's time per block)
        // a unit pays for itself (a dozen dependent round trips before its first block, its own heap to warm up): below a few
        // dozen blocks that is most of its time. The floor only binds for small batches -- the per-GPU share of a batch sharded over 8 GPUs
        const double floor_cost = (rmw_cost && c <= 2) ? 256.0 : 48.0;
        const double target = std::max(floor_cost, all_cost / (unit_factor * resident) / (c == 0 ? 1.0 : 4.0) / (c == 3 && rmw_cost ? 4.0 : 1.0));
        ++b.nqcls[c];
        if (((r.and_stream && nt >= 2 && nt <= 4) || (r.list_stream && nt == 1)) && add_list_streams(b, ix, q, nt)) {
            b.q_unit_off[q + 1] = (uint32_t)b.units.size();
            continue;
        }
        if (r.seeded && nt == 1) { // one list: wand == maxscore == ranked_and, answered by the (block-synchronous) seed pass
            b.single_queries.push_back(q);
            b.q_unit_off[q + 1] = (uint32_t)b.units.size();
            continue;
        }
        if (c == CLS_LONG && !nt) {
            // an empty query of a k > 64 batch (Route::goes_long(0); the seed pass of a k > 64 union batch holds thousands of them): no
            // k_daat_long unit -- the rows are cleared before the kernels run, and an untouched row is the empty answer (count 0, length 0,
            // doc-ids 0xFFFFFFFF) but for its scores, which copy_results pads
            b.empty_queries.push_back(q);
        } else if (c == CLS_LONG) { // > 16 terms: one unit, reference-order traversal over global scratch
            add_unit(b, c, q, 0, r.conj ? std::max(1u, qnb0[q]) : (uint32_t)ix.num_docs, 1, qcost[q]);
        } else if (r.conj) {
            const uint32_t nb0 = std::max(1u, qnb0[q]);
            const bool taper = taper_batch && nt > 1;
            uint32_t parts = 1;
            if (split_ok && nt && qnb0[q] > 1) parts = ds2i_cut::equal_parts(nb0, qcost[q], taper ? std::max(target, unit_start_cost(nt)) : target);
            uint32_t cap_blocks = 0; // DS2I_UNIT_CAP: the blocks a unit may hold at most (0 = no bound)
            if (rmw_units && split_ok && nt > 1) {
                // The cost model prices a block of the driving list at its average, but a query whose conjunction holds fewer than k
                // documents never gets a threshold: every one of its blocks goes all the way through the other lists (10 us per
                // block with 2 lists, 25 us with 4, against 2-4 us). Left whole, a 600-block query of that kind ran for 6 ms and WAS
                // the kernel's span (DS2I_UNIT_CLOCK: 1 700 of 6 144 wave slots busy on average). The cost model above now prices
                // such queries; DS2I_UNIT_CAP (blocks; half of it beyond 2 lists) additionally bounds every unit -- off by
                // default: cutting EVERY query that fine cost 20 % (each part warms up its own heap). The tests use it to split everything.
                const uint32_t cap_env = ix.knobs->unit_cap;
                if (cap_env) {
                    cap_blocks = c == 0 ? cap_env : std::max(8u, cap_env / 2);
                    parts = std::max(parts, (nb0 + cap_blocks - 1) / cap_blocks);
                }
            }
            // `and` through the stream pipeline has no heap to warm up -- a part costs its blocks and nothing else -- and a two-list query
            // left whole was a single wave for up to 13 ms (DS2I_UNIT_CLOCK: class 0 = 487 units, median 4.9 ms, 229 waves busy on
            // average, the span of the whole batch): at most 96 blocks of the shortest list per unit
            if (r.and_rs_units && split_ok && nt > 1 && nt <= r.stream_nt_max) parts = std::max(parts, (nb0 + and_unit_blocks - 1) / and_unit_blocks);
            if (taper) {
                add_tapering_units(b, c, q, nb0, parts, cap_blocks, qcost[q], cut);
            } else { // parts of ceil(nb0 / parts) blocks each (= unit_cut.hpp's cut at ratio 1, without its boundary vector)
                const uint32_t per = (nb0 + parts - 1) / parts;
                parts = (nb0 + per - 1) / per;
                if (parts > 1) b.split_queries.push_back(q);
                for (uint32_t j = 0; j < parts; ++j) add_unit(b, c, q, j * per, std::min(nb0, (j + 1) * per), parts, qcost[q] / parts);
            }
        } else if (r.union_stream && !nt) { // empty query: one unit of an empty virtual query writes the empty answer
            b.voff.push_back((uint32_t)b.vterms.size());
            b.vinfo.push_back(q);
            b.vinfo.push_back(0);
            b.vinfo.push_back(0);
            add_unit(b, c, (uint32_t)b.voff.size() - 2, 0, 0, 1, 0.0);
        } else if (r.union_stream) {
            cut_union_query(b, q, c, ut_blocks);
        } else {
            // or / ranked_or / wand / maxscore: units are equal-width doc-id ranges; every part keeps its own
            // top-k (its own pruning threshold), the merge is exact
            const uint32_t N = (uint32_t)ix.num_docs;
            uint32_t parts = 1;
            // every part re-seeks its lists; how fine the parts should be cut per class was measured on the GOV2-scale
            // batch (wand, queries/s): {8,2,1,1} 50.6 k, {8,2,2,2} 54.5 k, {8,4,4,4} 55.4 k, {4,2,4,4} 55.7 k -- with the
            // shared score histogram a part no longer has to warm up its own threshold, so the latency-bound many-list
            // classes gain from finer parts
            static const double disj_scale[NCLS] = {4.0, 2.0, 4.0, 4.0, 1.0};
            // or / or_freq run as a stream (k_union): a part costs a positioning of every list plus its blocks, once each
            const bool stream_or = !r.ranked && !r.reference;
            const double dtarget = std::max(48.0, all_cost / (unit_factor * (stream_or ? 1.0 : disj_scale[c]) * resident));
            if (nt && N > 1)
                parts = (uint32_t)std::min<double>(std::max(1.0, std::floor(qcost[q] / dtarget)), std::min<double>(N, 1024.0));
            const uint32_t width = (N + parts - 1) / parts;
            parts = width ? (N + width - 1) / width : 1;
            if (parts > 1) b.split_queries.push_back(q);
            for (uint32_t j = 0; j < parts; ++j)
                add_unit(b, c, q, j * width, (uint32_t)std::min<uint64_t>(N, (uint64_t)(j + 1) * width), parts, qcost[q] / parts);
        }
        b.q_unit_off[q + 1] = (uint32_t)b.units.size();
    }
    b.nunits = (uint32_t)b.units.size();
    b.nsplit = (uint32_t)b.split_queries.size();
    b.nsingle = (uint32_t)b.single_queries.size();
}

// The units of class c stably partitioned by their list capacity (cap_of: 0 .. DS2I_HIP_MAX_TERMS + 1), largest first, and cut into
// one launch group per capacity: capacities 2 .. DS2I_HIP_MAX_TERMS run `stream` (the stream kernel compiled for that capacity), the
// others the class kernel with the class's list slots. Inside a group the units stay in cost order.
template <class CapOf>
void stream_groups(BatchPlan& b, int c, const CapOf& cap_of, uint32_t cls_lists, GroupKernel stream) {
    uint32_t cnt[DS2I_HIP_MAX_TERMS + 2] = {}; // stable partition by capacity, largest first
    for (uint32_t uid : b.order[c]) ++cnt[cap_of(uid)];
    uint32_t start[DS2I_HIP_MAX_TERMS + 2], acc = 0;
    for (int n = DS2I_HIP_MAX_TERMS + 1; n >= 0; --n) { start[n] = acc; acc += cnt[n]; }
    std::vector<uint32_t>& tmp = b.scratch_u32;
    tmp.resize(b.order[c].size());
    for (uint32_t uid : b.order[c]) tmp[start[cap_of(uid)]++] = uid;
    b.order[c].swap(tmp);
    for (uint32_t i = 0; i < b.ncls[c];) {
        uint32_t j = i;
        const uint32_t l = cap_of(b.order[c][i]);
        while (j < b.ncls[c] && cap_of(b.order[c][j]) == l) ++j;
        const bool s = l >= 2 && l <= DS2I_HIP_MAX_TERMS;
        b.sub[c].push_back({i, j, s ? l : cls_lists, s ? stream : GroupKernel::cls});
        i = j;
    }
}

// ---- launch groups: every class's units in cost order, cut into the groups its kernels are launched for
static int form_groups(BatchPlan& b, const PlanIndex& ix) {
    const Route& r = b.route;
    const std::vector<uint32_t>& qoff = b.qoff;
    for (int c = 0; c < NCLS; ++c) {
        order_by_cost(b.unit_cost, b.cls_units[c], b.order[c], b.scratch_u32); // costliest first
        b.ncls[c] = (uint32_t)b.order[c].size();
        b.sub[c].clear();
        if (!b.ncls[c]) continue;
        // Residency hides the union kernels' dependent round trips and LDS per wave caps it. The <=2- and <=4-list kernels
        // are capped by registers first (6 / 5 waves per SIMD), so only the many-list classes are cut into groups: the
        // longest queries first, costliest first inside a group (stable). The groups of a class run back to back on its
        // stream, so finer is not better: granularity in lists, measured on the GOV2-scale wand batch (round 2: k_disjunctive)
        // 0 (off) 60.6 k, 1: 60.0 k, 2: 62.4 k, 4: 61.0 k queries/s.
        const uint32_t dyn_group = 2u;
        const uint32_t cls_lists = c == 0 ? 2u : c == 1 ? 4u : c == 2 ? 8u : 16u;
        const bool union_kernel = !r.conj && !r.reference && c != CLS_LONG;
        const int dyn_mincls = 2;
        if (r.union_stream) {
            // block_optpfor with every upload-time table: the virtual queries of 2 .. 8 lists run the pipelined stream kernel compiled for
            // exactly their list count (union_stream.hip), one launch group per count, back to back on the class stream -- as ranked_and
            // does (below); everything else (other codecs, 9-16 lists, the empty query's unit): k_union_topk, static LDS, one launch per class
            if (!(r.us_ok && c <= 3)) {
                b.sub[c].push_back({0u, b.ncls[c], cls_lists, GroupKernel::cls});
                continue;
            }
            // (list CAPACITIES 2 | 4 | 6 | 8 | 16: a launch group holds the virtual queries of cap - 1 and cap (9 .. 16) lists -- five groups
            // and five tails per batch; inside a group the units stay in cost order)
            auto cap_of = [&](uint32_t uid) { const uint32_t vq = b.units[uid].q, n = b.voff[vq + 1] - b.voff[vq]; return n < 2 ? 0u : n > DS2I_HIP_MAX_TERMS ? DS2I_HIP_MAX_TERMS + 1u : n > 8 ? (uint32_t)DS2I_HIP_MAX_TERMS : (n + 1u) & ~1u; };
            stream_groups(b, c, cap_of, cls_lists, r.bigk ? GroupKernel::union_stream_bigk : GroupKernel::union_stream);
            continue;
        }
        if (r.rs_ok && (uint32_t)c < r.rs_classes) {
            // launch groups by list CAPACITY 2 | 4 | 6 | 8 (block_optpfor: a group holds the queries of cap - 1 and cap lists, UnitRec::pad says
            // which; block_mixed native: the exact count, 2 .. 4): four groups and four tails per batch instead of seven; queries beyond
            // DS2I_STREAM_NT_MAX lists and one-term queries form the class kernel's groups. Inside a group the units stay in cost order.
            auto cap_of = [&](uint32_t uid) {
                const uint32_t q = b.units[uid].q, n = qoff[q + 1] - qoff[q];
                if (n == 1 && r.bigk_stream) return 4u; // (k > 64: the one-term queries ride in the capacity-4 launch)
                return n < 2 ? n : n > r.rs_nt ? DS2I_HIP_MAX_TERMS + 1u : r.exact ? n : n > 8 ? (uint32_t)DS2I_HIP_MAX_TERMS : (n + 1u) & ~1u;
            };
            const GroupKernel kernel = (r.base_op == DS2I_OP_AND || r.base_op == DS2I_OP_AND_FREQ) ? GroupKernel::and_rstream
                                       : ix.kind == DS2I_BLOCK_MIXED                              ? GroupKernel::ranked_stream_mixed
                                       : r.bigk                                                     ? GroupKernel::ranked_stream_bigk
                                                                                                    : GroupKernel::ranked_stream;
            stream_groups(b, c, cap_of, cls_lists, kernel);
            continue;
        }
        if (union_kernel && !r.ranked) { // or / or_freq: the streaming kernel serves every list count (lists = ~0 says so)
            b.sub[c].push_back({0u, b.ncls[c], 0xFFFFFFFFu, GroupKernel::cls});
            continue;
        }
        if (!union_kernel || c < dyn_mincls || dyn_group == 0) {
            b.sub[c].push_back({0u, b.ncls[c], cls_lists, GroupKernel::cls});
            continue;
        }
        auto lists_of = [&](uint32_t uid) {
            const uint32_t q = b.units[uid].q, n = qoff[q + 1] - qoff[q];
            const uint32_t g = c == 1 ? 1u : dyn_group; // (3- and 4-list queries: exact)
            return std::min(cls_lists, (n + g - 1) / g * g);
        };
        std::stable_sort(b.order[c].begin(), b.order[c].end(), [&](uint32_t x, uint32_t y) { return lists_of(x) > lists_of(y); });
        for (uint32_t i = 0; i < b.ncls[c];) {
            uint32_t j = i;
            const uint32_t l = lists_of(b.order[c][i]);
            while (j < b.ncls[c] && lists_of(b.order[c][j]) == l) ++j;
            // a group narrower than one of its queries would make the kernel answer that query with an empty result
            for (uint32_t t = i; t < j; ++t) {
                const uint32_t q = b.units[b.order[c][t]].q;
                if (qoff[q + 1] - qoff[q] > l) return fail(b, DS2I_EINVAL, "internal: launch group has fewer list slots than a query of it");
            }
            b.sub[c].push_back({i, j, l, GroupKernel::cls});
            i = j;
        }
    }
    return DS2I_OK;
}

// ---- layouts: the upload block, the result block and the device scratch of the batch
static void lay_out(BatchPlan& b, const PlanIndex& ix) {
    const Route& r = b.route;
    const uint32_t nq = b.nq, k = b.k;
    size_t o = 0;
    auto place = [&](size_t bytes) { size_t at = o; o = align16(o + bytes); return at; };
    if (r.union_stream) { // the kernels see the virtual queries; the per-query arrays (units by query, histogram slots) stay real
        b.qterms.swap(b.vterms);
        b.qoff.swap(b.voff);
    }
    b.o_qterms = place(b.qterms.size() * sizeof(QTerm));
    b.o_qoff = place(b.qoff.size() * 4);
    b.o_vinfo = place(r.union_stream ? b.vinfo.size() * 4 : 0);
    b.o_units = place(b.units.size() * sizeof(Unit));
    b.o_q_unit_off = place(b.q_unit_off.size() * 4);
    b.o_split = place(b.split_queries.size() * 4);
    b.o_single = place(b.single_queries.size() * 4);
    b.hist_slot.assign(nq ? nq : 1, 0xFFFFFFFFu); // a split query's score histogram = its rank among the split queries
    for (uint32_t i = 0; i < b.nsplit; ++i) b.hist_slot[b.split_queries[i]] = i;
    b.o_hslot = place(b.hist_slot.size() * 4);
    for (int c = 0; c < NCLS; ++c) b.o_order[c] = place(b.order[c].size() * 4);
    for (int c = 0; c < 4; ++c) b.o_urec[c] = place(c < r.urec_classes() ? b.order[c].size() * sizeof(ds2i_dev::UnitRec) : 0);
    b.o_qterm_q = place(r.freq_stream ? b.qterms.size() * 4 : 0);
    b.o_sterms = place(b.sterms.size() * sizeof(ds2i_dev::StreamTerm));
    b.o_match_off = place(b.want_matches ? b.match_off.size() * 8 : 0);
    b.up_bytes = o + 16;
    const size_t nq1 = nq ? nq : 1, nu1 = b.nunits ? b.nunits : 1;
    o = 0;
    b.o_count = place(8 * nq1);
    b.o_topk = place(4 * nq1 * k);
    b.o_topk_len = place(4 * nq1);
    b.o_freq_sum = place(8 * nq1);
    b.o_topk_docs = place(r.docs ? 4 * nq1 * k : 0); // (DS2I_OP_TOPK_DOCS; last, so the scores-only layout is unchanged)
    b.out_bytes = o;
    o = 0;
    b.o_unit_count = place(8 * nu1);
    b.o_unit_topk = place(4 * nu1 * k);
    b.o_unit_topk_len = place(4 * nu1);
    b.o_unit_freq_sum = place(8 * nu1);
    b.o_unit_topk_docs = place(r.docs ? 4 * nu1 * k : 0);
    // ranked_and / wand / maxscore / ranked_or: a 256-bucket score histogram per split query (kernels.hip, ScoreHist)
    b.hist = !r.reference && b.nsplit && ((r.base_op == DS2I_OP_RANKED_AND && ix.bmw) || r.disj_topk);
    b.o_qfloor = place(b.hist ? 1024 * (size_t)b.nsplit : 16);
    b.o_qfloorw = place(b.hist ? 4 * (size_t)b.nsplit : 16); // k_ranked_stream: the floor the histogram implies, one word per split query
    b.scr_bytes = o;
}

// ---- the seed pass (wand / maxscore / ranked_or): a ranked_and batch of its own over sub-queries of the same queries (seed_request)
static void plan_seed(BatchPlan& b, const PlanIndex& ix, const uint32_t* terms, const uint32_t* query_offsets) {
    const uint32_t nq = b.nq;
    // The seed is the ranked_and top-k of a SUB-query: any k documents' partial scores bound the final k-th
    // score from below. One- and two-term queries use all their terms (the one-term answer is final); longer
    // queries use their two shortest lists -- the full conjunction of 5+ terms is usually too small to give k
    // documents, while the rarest pair is cheap to intersect and carries the largest term weights.
    const size_t seed_terms = 2;
    // The streams (k_union_topk) start from the static floor and share a score histogram per query: measured on the
    // GOV2-scale wand batch the sub-query pass costs 8.3 ms to save 17 % of the block decodes (209 k queries/s with it,
    // 278 k without), so there only the one-term queries keep it -- it is what answers them.
    const bool seed_single_only = b.route.union_stream;
    auto& sterms = b.seed_terms;
    auto& soffs = b.seed_offs;
    sterms.clear();
    soffs.assign(nq + 1, 0);
    std::vector<uint32_t> dt;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t* qb = terms + query_offsets[q];
        const uint32_t* qe = terms + query_offsets[q + 1];
        dt.assign(qb, qe);
        std::sort(dt.begin(), dt.end());
        dt.erase(std::unique(dt.begin(), dt.end()), dt.end());
        if (seed_single_only && dt.size() > 1) {
            // no sub-query: the stream kernels find their floor themselves (static floor + shared histogram)
        } else if (dt.size() > seed_terms && dt.size() > 2) {
            std::stable_sort(dt.begin(), dt.end(), [&](uint32_t x, uint32_t y) { return ix.list_n[x] < ix.list_n[y]; });
            dt.resize(std::max<size_t>(2, seed_terms));
            for (const uint32_t* p = qb; p != qe; ++p) // keep multiplicities: the query term weight counts them
                if (std::find(dt.begin(), dt.end(), *p) != dt.end()) sterms.push_back(*p);
        } else {
            sterms.insert(sterms.end(), qb, qe);
        }
        soffs[q + 1] = (uint32_t)sterms.size();
    }
}

} // namespace

// (the plan's vectors grow with the batch: an allocation failure -- on the caller's thread or on a pool thread, see PlanPool -- is
// an error code at the C boundary, not an exception crossing it)
int plan_batch(BatchPlan& b, const PlanIndex& ix, const PlanRequest& rq) {
    const auto plan_t0 = std::chrono::steady_clock::now();
    const uint32_t nq = rq.nq;
    b.rc = DS2I_OK;
    b.err.clear();
    if (!rq.query_offsets || (!rq.terms && nq && rq.query_offsets[nq] > 0))
        return fail(b, DS2I_EINVAL, "ds2i_hip_batch_prepare: null argument");
    try {
        double all_cost = 0;
        int rc = plan_route(b, ix, rq);
        if (!rc) rc = plan_queries(b, ix, rq.terms, rq.query_offsets, all_cost);
        if (rc) return rc;
        cut_units(b, ix, all_cost);
        rc = form_groups(b, ix);
        if (rc) return rc;
        if (ix.knobs->unit_clock) // (diagnostic)
            std::fprintf(stderr, "ds2i plan: op %d nq %u units %u (per class %u %u %u %u %u) split queries %u cost %.0f, %.0f us\n", rq.op, nq, b.nunits,
                         b.ncls[0], b.ncls[1], b.ncls[2], b.ncls[3], b.ncls[4], b.nsplit, all_cost,
                         1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - plan_t0).count());
        lay_out(b, ix);
        b.use_seed = b.route.seeded && nq;
        if (b.use_seed) plan_seed(b, ix, rq.terms, rq.query_offsets);
        return DS2I_OK;
    } catch (std::bad_alloc const&) {
        return fail(b, DS2I_ENOMEM, "out of host memory planning the batch");
    } catch (std::exception const& e) {
        return fail(b, DS2I_EINVAL, e.what());
    }
}

PlanRequest seed_request(const BatchPlan& b) {
    PlanRequest s;
    // (a docs batch's seed runs with doc-ids too: it answers the one-term queries, k_copy_seed_docs)
    s.op = DS2I_OP_RANKED_AND | (b.route.docs ? (int)DS2I_OP_TOPK_DOCS : 0);
    s.k = b.k;
    s.terms = b.seed_terms.data();
    s.query_offsets = b.seed_offs.data();
    s.nq = b.nq;
    s.pool_batches = b.pool_batches;
    s.no_bigk_streams = b.no_bigk_streams;
    return s;
}

// ---------------------------------------------------------------- the upload block: every byte the kernels read of a plan (lay_out)
void pack_upload(const BatchPlan& b, uint8_t* h) {
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(h + off, src, bytes); };
    put(b.o_qterms, b.qterms.data(), b.qterms.size() * sizeof(QTerm));
    put(b.o_qoff, b.qoff.data(), b.qoff.size() * 4);
    if (b.route.union_stream) put(b.o_vinfo, b.vinfo.data(), b.vinfo.size() * 4);
    put(b.o_units, b.units.data(), b.units.size() * sizeof(Unit));
    put(b.o_q_unit_off, b.q_unit_off.data(), b.q_unit_off.size() * 4);
    put(b.o_split, b.split_queries.data(), b.split_queries.size() * 4);
    put(b.o_single, b.single_queries.data(), b.single_queries.size() * 4);
    put(b.o_hslot, b.hist_slot.data(), b.hist_slot.size() * 4);
    for (int c = 0; c < NCLS; ++c) put(b.o_order[c], b.order[c].data(), b.order[c].size() * 4);
    put(b.o_sterms, b.sterms.data(), b.sterms.size() * sizeof(ds2i_dev::StreamTerm));
    if (b.route.freq_stream) { // or_freq: the query of every term (k_freq_stream adds a term's freqs to its query's checksum)
        uint32_t* qq = (uint32_t*)(h + b.o_qterm_q);
        for (uint32_t q = 0; q < b.nq; ++q)
            for (uint32_t i = b.qoff[q]; i < b.qoff[q + 1]; ++i) qq[i] = q;
    }
    // one record per ticket: what k_ranked_stream / k_union_stream read where a unit starts -- the unit, its query's terms, its query
    // (k_union_stream: its virtual query's terms, its REAL query -- results, histogram -- and its exclusion lists)
    const bool vq = b.route.union_stream;
    for (int c = 0; c < b.route.urec_classes(); ++c) {
        ds2i_dev::UnitRec* r = (ds2i_dev::UnitRec*)(h + b.o_urec[c]);
        for (size_t i = 0; i < b.order[c].size(); ++i) {
            const uint32_t uid = b.order[c][i];
            const Unit& u = b.units[uid];
            const uint32_t rq = vq ? b.vinfo[3 * (size_t)u.q] : u.q, nt = b.qoff[u.q + 1] - b.qoff[u.q];
            r[i] = ds2i_dev::UnitRec{uid, rq, u.blk_begin, u.blk_end, u.nparts, b.qoff[u.q], b.hist_slot[rq], vq ? b.vinfo[3 * (size_t)u.q + 1] | (nt << 8) : nt};
        }
    }
    if (b.want_matches) put(b.o_match_off, b.match_off.data(), b.match_off.size() * 8);
}
