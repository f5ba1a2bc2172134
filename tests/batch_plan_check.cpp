// Stand-alone check of the batch planner (ds2i_amd/csrc/batch_plan.{hpp,cpp}; its own main, no HIP): batches planned over a fabricated
// PlanIndex -- the 24 list lengths of tests/batch_size_cases.py over 2^17 documents, five capability variants, 8 and 256 compute units --
// and every plan held to what the slot, the launchers and the kernels trust of it: each query answered one way, the unit cover, the
// class and group bookkeeping, the byte layout of the three blocks, the packed upload block, the seed pass, determinism over planning
// threads and over reuse of a BatchPlan, and the error codes. Built with -fsanitize=address,undefined and with -fsanitize=thread and
// run by tests/test_batch_plan_cpu.py. Prints "batch_plan: N plans hold" and returns 0; the first failing case is printed with its
// parameters and the exit status is 1. With --digests every plan's digest is printed as well (one line per case); --threaded keeps to
// what the planning threads take part in -- the error cases, the 36 000-query batches and the comparison over thread counts -- and compares
// digests without the other checks (the thread sanitizer's run); --probe only starts.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../ds2i_amd/csrc/batch_plan.hpp"

using ds2i_dev::QTerm;
using ds2i_dev::StreamTerm;
using ds2i_dev::Unit;
using ds2i_dev::UnitRec;

// ---------------------------------------------------------------- the fabricated index
static const uint32_t NUM_DOCS = 1u << 17;
static const uint32_t LIST_SIZES[24] = {3, 17, 40, 64, 127, 128, 129, 200, 300, 513, 650, 777, 900, 2047, // sparse: no bitmap
                                        2048, 2300, 2700, 3100, 3600, 4096,                               // dense
                                        23000, 34000, 46000, 58000};                                      // long: 180 .. 454 blocks
enum Variant { OPTPFOR_ALL, OPTPFOR_NONE, MIXED_SKIP, OPT, NO_WAND, NVARIANTS };
static const char* const VARIANT_NAME[] = {"block_optpfor+tables", "block_optpfor bare", "block_mixed native+skip", "opt", "no wand"};

struct Fab {
    std::vector<QTerm> proto;
    std::vector<uint32_t> n;
    std::vector<float> topbmw;
    Ds2iKnobs knobs{};
    PlanIndex ix;
};

// nlists lists (list t as long as LIST_SIZES[t % 24]), nblocks = ceil(n / 128), positive weights, list_topbmw descending
static void fabricate(Fab& f, Variant v, int num_cus, unsigned plan_threads, uint32_t nlists = 24) {
    f.proto.assign(nlists, QTerm{});
    f.n.assign(nlists, 0);
    f.topbmw.assign((size_t)nlists * DS2I_HIP_MAX_K, 0.f);
    uint64_t off = 0, blk = 0, tail = 0, rmw64 = 0;
    for (uint32_t t = 0; t < nlists; ++t) {
        const uint32_t n = LIST_SIZES[t % 24], nb = (n + 127) / 128;
        QTerm& q = f.proto[t];
        q.list_off = off;
        off += 5 + 3 * (uint64_t)n;
        q.list_end = off;
        q.n = n;
        q.q_weight = 0.5f + 0.015625f * (float)(t % 24);   // (parked: max_term_weight)
        q.max_weight = 0.875f - 0.0078125f * (float)(t % 7); // (parked: the list's largest block weight)
        q.term = v == OPT ? nb : t;
        q.aux0 = v == OPT ? 64 * off : blk;
        q.aux1 = v == OPT ? 64 * off + 32 : tail;
        q.blk_base = (uint32_t)blk;
        uint32_t shift = 0;
        while (shift < 31 && ((uint64_t)NUM_DOCS >> (shift + 1)) >= 4ull * n) ++shift; // about 4 entries per posting
        q.rmw_off64 = (uint32_t)rmw64;
        q.rmw_shift = shift;
        q.nblocks = nb;
        rmw64 += (ds2i_dev::RmwLevels(NUM_DOCS, shift).bytes() + ds2i_dev::RmwLevels::bitmap_bytes(NUM_DOCS)) / 64;
        blk += nb;
        tail += n % 128;
        f.n[t] = n;
        for (uint32_t j = 0; j < DS2I_HIP_MAX_K && j < nb; ++j) f.topbmw[(size_t)t * DS2I_HIP_MAX_K + j] = q.max_weight * (1.0f - (float)j / 128.0f);
    }
    std::memset(&f.knobs, 0, sizeof f.knobs);
    f.knobs.rmw_g = 4.0;
    f.knobs.ut_blocks = 320;
    f.knobs.stream_nt_max = 16;
    f.knobs.plan_threads = plan_threads;
    PlanIndex& ix = f.ix;
    ix = PlanIndex{};
    ix.kind = v == MIXED_SKIP ? DS2I_BLOCK_MIXED : v == OPT ? DS2I_OPT : DS2I_BLOCK_OPTPFOR;
    ix.num_cus = num_cus;
    ix.size = nlists;
    ix.num_docs = NUM_DOCS;
    ix.has_wand = v != NO_WAND;
    ix.skip = v == OPTPFOR_ALL || v == MIXED_SKIP || v == NO_WAND;
    ix.bmw = ix.rmw = v == OPTPFOR_ALL || v == MIXED_SKIP || v == OPT;
    ix.has_bitmaps = ix.rmw;
    ix.side_tables = v == OPTPFOR_ALL || v == NO_WAND;
    ix.bound_tables = ix.bmw && ix.rmw;
    ix.skip_or_pef = ix.skip || ix.kind >= DS2I_OPT;
    ix.knobs = &f.knobs;
    ix.term_proto = f.proto.data();
    ix.list_n = f.n.data();
    ix.list_topbmw = f.topbmw.data();
}

// ---------------------------------------------------------------- queries and batches
typedef std::vector<uint32_t> Query;

static std::vector<Query> query_pool() {
    std::vector<Query> qs;
    qs.push_back({});                                           // the empty query
    for (uint32_t n = 1; n <= 17; ++n) {                        // every length 1 .. 17
        Query q;
        for (uint32_t i = 0; i < n; ++i) q.push_back((5 * n + 7 * i) % 24); // (7 and 24 are coprime: distinct terms)
        qs.push_back(q);
    }
    Query q20;
    for (uint32_t t = 2; t < 22; ++t) q20.push_back(t);         // 20 terms, one of them twice
    q20.push_back(7);
    qs.push_back(q20);
    for (Query q : {Query{5, 5}, Query{3, 9, 3}, Query{20, 13, 20, 13}, Query{14, 14, 17}, Query{21, 21}}) qs.push_back(q); // duplicated terms
    for (Query q : {Query{14, 15}, Query{16, 19}, Query{14, 16, 18}, Query{14, 15, 16, 17}}) qs.push_back(q);               // all dense, 2 .. 4
    for (Query q : {Query{12, 19}, Query{0, 14}, Query{9, 16, 18}, Query{4, 17, 18, 19}, Query{11, 12}, Query{2, 3}}) qs.push_back(q); // sparse heads
    for (Query q : {Query{20, 21}, Query{22, 23}, Query{20, 23}, Query{20, 21, 22}, Query{20, 21, 22, 23}, Query{13, 23}, Query{19, 22},
                    Query{20}, Query{23}, Query{14}, Query{20, 21, 22, 23, 19}, Query{13, 20, 21, 22, 23, 18}})
        qs.push_back(q);                                        // over the long lists
    return qs;
}

struct Batch {
    std::vector<uint32_t> terms, offs;
    std::vector<uint32_t> pick; // pool index per query
};

// query i of the batch = pool[(first + a seeded walk) % pool]; one- and two-query batches start at `first`
static Batch make_batch(const std::vector<Query>& pool, uint32_t nq, uint32_t first) {
    Batch b;
    b.offs.push_back(0);
    uint64_t s = 0x9E3779B97F4A7C15ull ^ ((uint64_t)nq << 20);
    for (uint32_t i = 0; i < nq; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t p = nq <= 2 ? (first + i) % (uint32_t)pool.size() : (uint32_t)((s >> 33) % pool.size());
        b.pick.push_back(p);
        b.terms.insert(b.terms.end(), pool[p].begin(), pool[p].end());
        b.offs.push_back((uint32_t)b.terms.size());
    }
    if (b.terms.empty()) b.terms.push_back(0);
    return b;
}

// ---------------------------------------------------------------- planning through the planner's interface
struct Slot { BatchPlan plan, seed; };

static int plan_slot(Slot& s, const PlanIndex& ix, const PlanRequest& rq) {
    int rc = plan_batch(s.plan, ix, rq);
    if (!rc && s.plan.use_seed) rc = plan_batch(s.seed, ix, seed_request(s.plan));
    return rc;
}
static const BatchPlan& seed_of(const Slot& s) { return s.seed; }
static void packed(const BatchPlan& b, std::vector<uint8_t>& buf) {
    buf.assign(b.up_bytes, 0);
    pack_upload(b, buf.data());
}

// ---------------------------------------------------------------- digest (FNV-1a) of what a plan hands on
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void u64(uint64_t v) { h ^= v; h *= 1099511628211ull; }
    void bytes(const void* p, size_t n) { // (eight bytes a step: the blocks are megabytes)
        size_t i = 0;
        for (uint64_t w; i + 8 <= n; i += 8) { std::memcpy(&w, (const uint8_t*)p + i, 8); u64(w); }
        for (; i < n; ++i) u64(((const uint8_t*)p)[i]);
    }
};
static uint64_t digest_one(const BatchPlan& b) {
    std::vector<uint8_t> buf;
    packed(b, buf);
    Fnv f;
    f.bytes(buf.data(), buf.size());
    for (int c = 0; c < NCLS; ++c) {
        f.u64(b.sub[c].size());
        for (const SubLaunch& sl : b.sub[c]) { f.u64(sl.begin); f.u64(sl.end); f.u64(sl.lists); f.u64((uint64_t)sl.kernel); }
        f.u64(b.ncls[c]);
        f.u64(b.nqcls[c]);
        f.u64(b.o_order[c]);
    }
    for (int c = 0; c < 4; ++c) f.u64(b.o_urec[c]);
    for (size_t o : {b.o_vinfo, b.o_qterms, b.o_qoff, b.o_units, b.o_q_unit_off, b.o_split, b.o_single, b.o_hslot, b.o_qterm_q, b.o_sterms, b.o_match_off, b.up_bytes,
                     b.o_count, b.o_topk, b.o_topk_len, b.o_freq_sum, b.o_topk_docs, b.out_bytes, b.o_unit_count, b.o_unit_topk, b.o_unit_topk_len,
                     b.o_unit_freq_sum, b.o_unit_topk_docs, b.o_qfloor, b.o_qfloorw, b.scr_bytes})
        f.u64(o);
    for (uint64_t v : {(uint64_t)b.nunits, (uint64_t)b.nsplit, (uint64_t)b.nsingle, (uint64_t)b.long_terms, (uint64_t)b.sterm_longest, (uint64_t)b.sterms.size(),
                       (uint64_t)b.empty_queries.size(), (uint64_t)b.op, (uint64_t)b.k, (uint64_t)b.nq, (uint64_t)b.want_matches, (uint64_t)b.use_seed})
        f.u64(v);
    for (uint32_t q : b.empty_queries) f.u64(q);
    return f.h;
}
static uint64_t digest(const Slot& s) {
    Fnv f;
    f.u64(digest_one(s.plan));
    if (s.plan.use_seed) f.u64(digest_one(seed_of(s)));
    return f.h;
}

// ---------------------------------------------------------------- the checks
struct Case {
    Variant v;
    int num_cus;
    unsigned threads;
    int op;
    uint32_t k, nq, first;
    int want_matches;
    uint32_t pool_batches;
    bool no_list_streams, no_bigk_streams;
};
static std::string describe(const Case& c) {
    char s[320];
    std::snprintf(s, sizeof s, "index %s, %d CUs, plan_threads %u, op 0x%x, k %u, nq %u (first %u), want_matches %d, pool_batches %u, no_list_streams %d, no_bigk_streams %d",
                  VARIANT_NAME[c.v], c.num_cus, c.threads, c.op, c.k, c.nq, c.first, c.want_matches, c.pool_batches, (int)c.no_list_streams, (int)c.no_bigk_streams);
    return s;
}
static const Case* g_case = nullptr;
[[noreturn]] static void fail(const char* what, long long a = -1, long long b = -1) {
    std::printf("batch_plan FAILED: %s (%lld, %lld)\n  case: %s\n", what, a, b, g_case ? describe(*g_case).c_str() : "-");
    std::exit(1);
}
#define REQUIRE(cond, what, ...) do { if (!(cond)) fail(what, ##__VA_ARGS__); } while (0)

static inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

struct Region { size_t off, bytes; };
// every region 16-byte aligned, inside [0, total), in increasing order and disjoint
static void check_regions(const std::vector<Region>& rs, size_t total, const char* what) {
    size_t end = 0;
    for (const Region& r : rs) {
        REQUIRE(r.off % 16 == 0, what, (long long)r.off, 16);
        REQUIRE(r.off >= end, what, (long long)r.off, (long long)end);
        REQUIRE(r.off + r.bytes <= total, what, (long long)(r.off + r.bytes), (long long)total);
        end = r.off + r.bytes;
    }
}

// the cost key order_by_cost sorts by: descending, so the raw key must not increase
static uint32_t cost_key(float c) {
    uint32_t bits;
    c = c > 0.f ? c : 0.f;
    std::memcpy(&bits, &c, 4);
    return bits >> 17;
}

static void check_plan(const Slot& slot, const Fab& fab, const Batch& batch, const std::vector<Query>& pool, const Case& cs) {
    const BatchPlan& b = slot.plan;
    const Route& r = b.route;
    const uint32_t nq = cs.nq;
    const int base_op = cs.op & 0xFF;
    REQUIRE(b.nq == nq && b.op == cs.op && r.base_op == base_op, "plan header");
    REQUIRE(b.k == (base_op >= DS2I_OP_RANKED_AND ? cs.k : 1u), "k of the plan", b.k);
    // (lay_out: the kernels of the union streams see the virtual queries; the real ones are then in vterms / voff)
    const std::vector<uint32_t>& rqoff = r.union_stream ? b.voff : b.qoff;
    const std::vector<uint32_t>& kqoff = b.qoff;
    REQUIRE(rqoff.size() == (size_t)nq + 1, "query offsets", (long long)rqoff.size());
    // the distinct terms of every query, as the input has them
    std::vector<uint32_t> nt(nq), nb0(nq), pool_nt, pool_nb0;
    for (const Query& p : pool) {
        const std::set<uint32_t> d(p.begin(), p.end());
        uint32_t nmin = 0xFFFFFFFFu;
        for (uint32_t t : d) nmin = std::min(nmin, fab.n[t]);
        pool_nt.push_back((uint32_t)d.size());
        pool_nb0.push_back(d.empty() ? 0 : (nmin + 127) / 128); // blocks of the shortest list
    }
    for (uint32_t q = 0; q < nq; ++q) {
        nt[q] = pool_nt[batch.pick[q]];
        nb0[q] = pool_nb0[batch.pick[q]];
        REQUIRE(rqoff[q + 1] - rqoff[q] == nt[q], "terms kept of a query", q, rqoff[q + 1] - rqoff[q]);
    }
    // ---- each query is answered exactly one way
    REQUIRE(b.q_unit_off.size() == (size_t)nq + 1 && b.q_unit_off[0] == 0 && (nq == 0 || b.q_unit_off[nq] == b.units.size()), "q_unit_off ends");
    REQUIRE(b.nunits == b.units.size() && b.nsplit == b.split_queries.size() && b.nsingle == b.single_queries.size(), "counts of units / split / single");
    std::vector<uint32_t> streams(nq, 0), single(nq, 0), empty(nq, 0);
    for (const StreamTerm& st : b.sterms) {
        REQUIRE(st.q < nq, "list-stream record of no query", st.q);
        streams[st.q] += st.counts == 1 ? 1u : 0u;
        REQUIRE(st.counts <= 1 && st.nother + 1 == nt[st.q], "list-stream record", st.q);
    }
    for (const StreamTerm& st : b.sterms) REQUIRE(streams[st.q] == 1, "list-stream records without exactly one counting record", st.q);
    for (uint32_t q : b.single_queries) { REQUIRE(q < nq, "single query", q); ++single[q]; }
    for (uint32_t q : b.empty_queries) { REQUIRE(q < nq, "empty query", q); ++empty[q]; }
    uint32_t nqcls[NCLS] = {}, nsplit = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        REQUIRE(b.q_unit_off[q] <= b.q_unit_off[q + 1], "q_unit_off decreases", q);
        const uint32_t nu = b.q_unit_off[q + 1] - b.q_unit_off[q];
        REQUIRE((nu ? 1 : 0) + streams[q] + single[q] + empty[q] == 1, "a query is not answered exactly one way", q, nu);
        const int c = r.goes_long(nt[q]) ? CLS_LONG : class_of(nt[q]);
        ++nqcls[c];
        REQUIRE(!single[q] || (r.seeded && nt[q] == 1), "single query that is not a one-term query of a seeded batch", q);
        REQUIRE(!(r.seeded && nt[q] == 1) || single[q], "one-term query of a seeded batch not among the single queries", q);
        REQUIRE(!empty[q] || (nt[q] == 0 && c == CLS_LONG), "empty_queries holds a query with terms", q);
        // ---- cover
        const uint32_t u0 = b.q_unit_off[q];
        if (r.union_stream && nu) {
            // the units of the query's virtual queries, one virtual query after the other, each a partition of its driving list's blocks
            uint32_t u = u0;
            while (u < u0 + nu) {
                const uint32_t v = b.units[u].q;
                REQUIRE((size_t)3 * v + 2 < b.vinfo.size() && b.vinfo[3 * (size_t)v] == q, "virtual query of another query", q, v);
                const uint32_t vn = kqoff[v + 1] - kqoff[v];
                REQUIRE(vn == nt[q], "virtual query with other lists than its query", q, vn);
                const uint32_t nbe = vn ? std::max(1u, b.qterms[kqoff[v]].nblocks) : 0u;
                uint32_t at = 0;
                do {
                    const Unit& un = b.units[u];
                    REQUIRE(un.q == v && un.blk_begin == at && (un.blk_end > at || nbe == 0) && un.nparts == nu, "unit of a virtual query", q, u);
                    at = un.blk_end;
                    ++u;
                } while (at < nbe && u < u0 + nu);
                REQUIRE(at == nbe, "a virtual query's units do not cover its driving list", q, at);
            }
        } else if (nu) {
            const uint32_t span = r.conj ? std::max(1u, nb0[q]) : NUM_DOCS;
            uint32_t at = 0;
            for (uint32_t u = u0; u < u0 + nu; ++u) {
                const Unit& un = b.units[u];
                REQUIRE(un.q == q && un.blk_begin == at && un.blk_end > at && un.nparts == nu, "unit of a query", q, u);
                at = un.blk_end;
            }
            REQUIRE(at == span, "a query's units do not cover it", q, at);
            REQUIRE(c != CLS_LONG || nu == 1, "a long query in parts", q, nu);
        }
        if (nu > 1) {
            REQUIRE(nsplit < b.split_queries.size() && b.split_queries[nsplit] == q, "split_queries misses a query of several units", q);
            REQUIRE(b.hist_slot[q] == nsplit, "hist_slot of a split query", q, b.hist_slot[q]);
            ++nsplit;
        } else {
            REQUIRE(b.hist_slot[q] == 0xFFFFFFFFu, "hist_slot of a whole query", q, b.hist_slot[q]);
        }
    }
    REQUIRE(nsplit == b.split_queries.size(), "split_queries holds a whole query", nsplit, (long long)b.split_queries.size());
    REQUIRE(b.hist_slot.size() == (nq ? nq : 1u), "hist_slot size");
    uint32_t nqsum = 0;
    for (int c = 0; c < NCLS; ++c) { REQUIRE(b.nqcls[c] == nqcls[c], "queries per class", c, b.nqcls[c]); nqsum += b.nqcls[c]; }
    REQUIRE(nqsum == nq, "nqcls does not add up to nq", nqsum);
    // ---- classes and groups
    auto real_query = [&](uint32_t uid) { return r.union_stream ? b.vinfo[3 * (size_t)b.units[uid].q] : b.units[uid].q; };
    auto lists_of = [&](uint32_t uid) { const uint32_t q = b.units[uid].q; return kqoff[q + 1] - kqoff[q]; };
    std::vector<char> seen(b.units.size(), 0);
    REQUIRE(b.unit_cost.size() == b.units.size(), "unit_cost size");
    for (int c = 0; c < NCLS; ++c) {
        REQUIRE(b.ncls[c] == b.order[c].size() && b.order[c].size() == b.cls_units[c].size(), "units per class", c);
        std::vector<uint32_t> x = b.order[c], y = b.cls_units[c];
        std::sort(x.begin(), x.end());
        std::sort(y.begin(), y.end());
        REQUIRE(x == y, "order is not a permutation of the class's units", c);
        for (uint32_t uid : y) {
            REQUIRE(uid < seen.size() && !seen[uid], "a unit in two classes", uid);
            seen[uid] = 1;
            const uint32_t n = nt[real_query(uid)];
            REQUIRE((r.goes_long(n) ? CLS_LONG : class_of(n)) == c, "a unit in the wrong class", uid, c);
        }
        uint32_t at = 0;
        for (const SubLaunch& sl : b.sub[c]) {
            REQUIRE(sl.begin == at && sl.end > sl.begin && sl.end <= b.ncls[c], "launch groups do not tile the class", c, sl.begin);
            at = sl.end;
            if (sl.kernel == GroupKernel::ranked_stream_mixed) REQUIRE(sl.lists >= 2 && sl.lists <= 4, "list count k_ranked_stream_mixed is not compiled for", c, sl.lists);
            else if (sl.kernel != GroupKernel::cls)
                REQUIRE(sl.lists == 2 || sl.lists == 4 || sl.lists == 6 || sl.lists == 8 || sl.lists == 16, "capacity the stream kernels are not compiled for", c, sl.lists);
            for (uint32_t i = sl.begin; i < sl.end; ++i) {
                const uint32_t uid = b.order[c][i];
                REQUIRE(c == CLS_LONG || lists_of(uid) <= sl.lists, "launch group with fewer list slots than a query of it", uid, sl.lists);
                REQUIRE(i == sl.begin || cost_key(b.unit_cost[uid]) <= cost_key(b.unit_cost[b.order[c][i - 1]]), "cost key increases inside a launch group", c, i);
            }
        }
        REQUIRE(at == b.ncls[c], "launch groups end before the class does", c, at);
    }
    for (char s : seen) REQUIRE(s, "a unit in no class");
    // ---- layout
    const size_t nq1 = nq ? nq : 1, nu1 = b.nunits ? b.nunits : 1, k = b.k;
    std::vector<Region> up = {{b.o_qterms, b.qterms.size() * sizeof(QTerm)}, {b.o_qoff, b.qoff.size() * 4}, {b.o_vinfo, r.union_stream ? b.vinfo.size() * 4 : 0},
                              {b.o_units, b.units.size() * sizeof(Unit)}, {b.o_q_unit_off, b.q_unit_off.size() * 4}, {b.o_split, b.split_queries.size() * 4},
                              {b.o_single, b.single_queries.size() * 4}, {b.o_hslot, b.hist_slot.size() * 4}};
    for (int c = 0; c < NCLS; ++c) up.push_back({b.o_order[c], b.order[c].size() * 4});
    for (int c = 0; c < 4; ++c) up.push_back({b.o_urec[c], c < r.urec_classes() ? b.order[c].size() * sizeof(UnitRec) : 0});
    up.push_back({b.o_qterm_q, r.freq_stream ? b.qterms.size() * 4 : 0});
    up.push_back({b.o_sterms, b.sterms.size() * sizeof(StreamTerm)});
    up.push_back({b.o_match_off, b.want_matches ? b.match_off.size() * 8 : 0});
    check_regions(up, b.up_bytes, "upload block region");
    check_regions({{b.o_count, 8 * nq1}, {b.o_topk, 4 * nq1 * k}, {b.o_topk_len, 4 * nq1}, {b.o_freq_sum, 8 * nq1}, {b.o_topk_docs, r.docs ? 4 * nq1 * k : 0}}, b.out_bytes,
                  "result block region");
    REQUIRE(b.hist == (!r.reference && b.nsplit && ((base_op == DS2I_OP_RANKED_AND && fab.ix.bmw) || (base_op >= DS2I_OP_WAND && base_op <= DS2I_OP_RANKED_OR))), "score histograms", b.hist);
    check_regions({{b.o_unit_count, 8 * nu1}, {b.o_unit_topk, 4 * nu1 * k}, {b.o_unit_topk_len, 4 * nu1}, {b.o_unit_freq_sum, 8 * nu1}, {b.o_unit_topk_docs, r.docs ? 4 * nu1 * k : 0},
                   {b.o_qfloor, b.hist ? 1024 * (size_t)b.nsplit : 16}, {b.o_qfloorw, b.hist ? 4 * (size_t)b.nsplit : 16}}, b.scr_bytes, "scratch block region");
    REQUIRE(b.want_matches == (cs.want_matches && base_op <= DS2I_OP_AND_FREQ), "want_matches");
    if (b.want_matches) {
        REQUIRE(b.sterms.empty() && b.match_off.size() == (size_t)nq + 1, "match offsets");
        for (uint32_t q = 0; q < nq; ++q) REQUIRE(b.match_off[q + 1] - b.match_off[q] == 128ull * nb0[q], "match capacity of a query", q);
    }
    // ---- the packed upload block
    std::vector<uint8_t> buf;
    packed(b, buf);
    auto same = [&](size_t off, const void* p, size_t bytes) { return bytes == 0 || std::memcmp(buf.data() + off, p, bytes) == 0; };
    REQUIRE(same(b.o_qterms, b.qterms.data(), b.qterms.size() * sizeof(QTerm)) && same(b.o_qoff, b.qoff.data(), b.qoff.size() * 4) &&
            same(b.o_units, b.units.data(), b.units.size() * sizeof(Unit)) && same(b.o_q_unit_off, b.q_unit_off.data(), b.q_unit_off.size() * 4) &&
            same(b.o_split, b.split_queries.data(), b.split_queries.size() * 4) && same(b.o_single, b.single_queries.data(), b.single_queries.size() * 4) &&
            same(b.o_hslot, b.hist_slot.data(), b.hist_slot.size() * 4) && same(b.o_sterms, b.sterms.data(), b.sterms.size() * sizeof(StreamTerm)),
            "packed arrays");
    if (r.union_stream) REQUIRE(same(b.o_vinfo, b.vinfo.data(), b.vinfo.size() * 4), "packed vinfo");
    if (b.want_matches) REQUIRE(same(b.o_match_off, b.match_off.data(), b.match_off.size() * 8), "packed match offsets");
    for (int c = 0; c < NCLS; ++c) REQUIRE(same(b.o_order[c], b.order[c].data(), b.order[c].size() * 4), "packed class order", c);
    for (int c = 0; c < r.urec_classes(); ++c) {
        for (size_t i = 0; i < b.order[c].size(); ++i) {
            UnitRec rec;
            std::memcpy(&rec, buf.data() + b.o_urec[c] + i * sizeof(UnitRec), sizeof rec);
            const uint32_t uid = b.order[c][i], rq = real_query(uid), n = lists_of(uid);
            const Unit& u = b.units[uid];
            REQUIRE(rec.uid == uid && rec.q == rq && rec.blk_begin == u.blk_begin && rec.blk_end == u.blk_end && rec.nparts == u.nparts, "unit record and its unit", c, (long long)i);
            REQUIRE(rec.qt_off == kqoff[u.q] && rec.hist_slot == b.hist_slot[rq], "unit record's terms / histogram", c, (long long)i);
            REQUIRE(rec.pad == (r.union_stream ? (b.vinfo[3 * (size_t)u.q + 1] | (n << 8)) : n), "unit record's list count", c, (long long)i);
        }
    }
    if (r.freq_stream)
        for (uint32_t q = 0; q < nq; ++q)
            for (uint32_t i = kqoff[q]; i < kqoff[q + 1]; ++i) {
                uint32_t got;
                std::memcpy(&got, buf.data() + b.o_qterm_q + 4 * (size_t)i, 4);
                REQUIRE(got == q, "qterm_q", i, got);
            }
    // ---- the seed pass
    REQUIRE(b.use_seed == (r.seeded && nq), "use_seed", b.use_seed);
    if (!r.seeded) REQUIRE(b.single_queries.empty(), "single queries without a seed pass");
    if (b.use_seed) {
        const BatchPlan& s = seed_of(slot);
        REQUIRE((s.op & 0xFF) == DS2I_OP_RANKED_AND && s.k == b.k && s.nq == nq && s.route.docs == r.docs && !s.use_seed, "the seed batch");
        REQUIRE(b.seed_offs.size() == (size_t)nq + 1 && b.seed_offs[nq] == b.seed_terms.size(), "seed offsets");
        for (uint32_t q = 0; q < nq; ++q) {
            const Query& full = pool[batch.pick[q]];
            for (uint32_t i = b.seed_offs[q]; i < b.seed_offs[q + 1]; ++i)
                REQUIRE(std::find(full.begin(), full.end(), b.seed_terms[i]) != full.end(), "seed sub-query with a term its query lacks", q, b.seed_terms[i]);
            if (nt[q] == 1) REQUIRE(b.seed_offs[q + 1] - b.seed_offs[q] == full.size(), "one-term query's seed is not the query", q);
        }
    }
}

// ---------------------------------------------------------------- the matrix
static unsigned long long g_plans = 0;
static bool g_digests = false;
static bool g_threaded = false; // --threaded: the planning threads' share -- the error cases, the largest batches and the thread counts; digests only
static Slot g_reused; // planned on again and again: what a plan leaves behind must not show in the next

static PlanRequest request_of(const Case& c, const Batch& b) {
    PlanRequest rq;
    rq.op = c.op;
    rq.k = c.k;
    rq.terms = b.terms.data();
    rq.query_offsets = b.offs.data();
    rq.nq = c.nq;
    rq.want_matches = c.want_matches;
    rq.pool_batches = c.pool_batches;
    rq.no_list_streams = c.no_list_streams;
    rq.no_bigk_streams = c.no_bigk_streams;
    return rq;
}

// plans the case on the reused slot, checks the plan, and compares its digest with a fresh slot's; returns the digest
static uint64_t run_case(const Case& c, const std::vector<Query>& pool, bool fresh_too) {
    g_case = &c;
    Fab fab;
    fabricate(fab, c.v, c.num_cus, c.threads);
    static Batch batch; // (the batch of the case before, where it is the same)
    static uint32_t batch_nq = 0xFFFFFFFFu, batch_first = 0;
    if (batch_nq != c.nq || batch_first != c.first) {
        batch = make_batch(pool, c.nq, c.first);
        batch_nq = c.nq;
        batch_first = c.first;
    }
    const PlanRequest rq = request_of(c, batch);
    const int rc = plan_slot(g_reused, fab.ix, rq);
    const bool ranked = (c.op & 0xFF) >= DS2I_OP_RANKED_AND;
    if (ranked && c.v == NO_WAND) { // (every other case of the matrix plans)
        REQUIRE(rc == DS2I_ENOWAND, "ranked operator without wand data", rc);
        if (g_digests) std::printf("%s: rc %d\n", describe(c).c_str(), rc);
        ++g_plans;
        return 0;
    }
    REQUIRE(rc == DS2I_OK, "the batch does not plan", rc);
    if (!g_threaded) check_plan(g_reused, fab, batch, pool, c);
    const uint64_t d = digest(g_reused);
    if (fresh_too && !g_threaded) {
        Slot fresh;
        REQUIRE(plan_slot(fresh, fab.ix, rq) == DS2I_OK, "the batch does not plan on a fresh BatchPlan");
        REQUIRE(digest(fresh) == d, "a reused BatchPlan plans differently from a fresh one");
    }
    if (c.op & DS2I_OP_TOPK_DOCS) { // the result layout with the doc-ids = the one without, plus a last region
        Slot plain;
        PlanRequest rp = rq;
        rp.op &= ~DS2I_OP_TOPK_DOCS;
        REQUIRE(plan_slot(plain, fab.ix, rp) == DS2I_OK, "the batch does not plan without DS2I_OP_TOPK_DOCS");
        const BatchPlan &a = plain.plan, &b = g_reused.plan;
        REQUIRE(a.o_count == b.o_count && a.o_topk == b.o_topk && a.o_topk_len == b.o_topk_len && a.o_freq_sum == b.o_freq_sum && b.o_topk_docs == a.out_bytes &&
                b.out_bytes == a.out_bytes + align16(4 * (size_t)(c.nq ? c.nq : 1) * b.k), "result layout with doc-ids");
    }
    if (g_digests) std::printf("%s: %016llx\n", describe(c).c_str(), (unsigned long long)d);
    ++g_plans;
    return d;
}

// a batch of 2048 queries on 4 planning threads with one bad query in the first, a middle or the last chunk
static void error_cases(const std::vector<Query>& pool) {
    struct Bad { const char* what; int expect; };
    const Bad bads[] = {{"term out of range", DS2I_ETERM}, {"decreasing offsets", DS2I_EINVAL}, {"too many distinct terms", DS2I_ETOOLONG}, {"k = 0", DS2I_EINVAL},
                        {"k > DS2I_HIP_MAX_K_LONG", DS2I_EINVAL}, {"ranked without wand data", DS2I_ENOWAND}, {"DS2I_OP_TOPK_DOCS on and", DS2I_EINVAL}};
    g_case = nullptr;
    for (int kind = 0; kind < 7; ++kind)
        for (uint32_t where : {0u, 1024u, 2047u}) {
            Fab fab;
            fabricate(fab, kind == 5 ? NO_WAND : OPTPFOR_ALL, 256, 4, 1100);
            Batch b = make_batch(pool, 2048, 0);
            int op = DS2I_OP_RANKED_AND;
            uint32_t k = 10;
            if (kind == 0) { // (the nearest query of that chunk that has a term)
                uint32_t q = where;
                while (b.offs[q] == b.offs[q + 1]) q = where == 2047 ? q - 1 : q + 1;
                b.terms[b.offs[q]] = 1100;
            }
            if (kind == 1) { // the offsets dip at `where`
                b.terms.insert(b.terms.begin(), 4, 0u);
                for (uint32_t& o : b.offs) o += 4;
                b.offs[where + 1] = b.offs[where] - 1;
            }
            if (kind == 2) { // query `where` replaced by one of 1025 distinct terms, at the end of the term array
                Batch g;
                g.offs.push_back(0);
                for (uint32_t q = 0; q < 2048; ++q) {
                    if (q == where) for (uint32_t t = 0; t <= DS2I_HIP_MAX_TERMS_LONG; ++t) g.terms.push_back(t);
                    else g.terms.insert(g.terms.end(), b.terms.begin() + b.offs[q], b.terms.begin() + b.offs[q + 1]);
                    g.offs.push_back((uint32_t)g.terms.size());
                }
                b = g;
            }
            if (kind == 3) k = 0;
            if (kind == 4) k = DS2I_HIP_MAX_K_LONG + 1;
            if (kind == 6) op = DS2I_OP_AND | DS2I_OP_TOPK_DOCS;
            PlanRequest rq;
            rq.op = op;
            rq.k = k;
            rq.terms = b.terms.data();
            rq.query_offsets = b.offs.data();
            rq.nq = 2048;
            const int rc = plan_batch(g_reused.plan, fab.ix, rq);
            if (rc != bads[kind].expect || g_reused.plan.rc != rc || g_reused.plan.err.empty()) {
                std::printf("batch_plan FAILED: %s at query %u gives %d (%s), not %d\n", bads[kind].what, where, rc, g_reused.plan.err.c_str(), bads[kind].expect);
                std::exit(1);
            }
            if (g_digests) std::printf("error case %s at query %u: rc %d\n", bads[kind].what, where, rc);
            ++g_plans;
        }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--probe") == 0) return std::printf("batch_plan: the program starts\n") < 0; // (does a sanitizer's runtime?)
    g_digests = argc > 1 && std::strcmp(argv[1], "--digests") == 0;
    g_threaded = argc > 1 && std::strcmp(argv[1], "--threaded") == 0;
    const std::vector<Query> pool = query_pool();
    const int OPS[8] = {DS2I_OP_AND, DS2I_OP_AND_FREQ, DS2I_OP_OR, DS2I_OP_OR_FREQ, DS2I_OP_RANKED_AND, DS2I_OP_WAND, DS2I_OP_MAXSCORE, DS2I_OP_RANKED_OR};
    const std::vector<uint32_t> ALL_SIZES = {0, 1, 2, 64, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4096, 4097};
    const std::vector<uint32_t> EDGE_SIZES = {0, 1, 2, 64, 512, 513, 1023, 1024, 1536, 2048, 4096, 4097}, FEW_SIZES = {1, 64, 513, 1535, 2049, 4096};
    const uint32_t npool = (uint32_t)pool.size();
    auto ranked = [](int op) { return (op & 0xFF) >= DS2I_OP_RANKED_AND; };
    unsigned long long n = 0;
    auto run = [&](Case c) { // (a fresh BatchPlan beside the reused one: every batch of 64 .. 1025 queries and every fifth other one)
        if (!ranked(c.op)) c.k = 0;
        return run_case(c, pool, (c.nq >= 64 && c.nq <= 1025) || ++n % 5 == 0);
    };
    if (g_threaded) error_cases(pool);
    else {
        // Every operator at k = 10 on every index and both machine sizes. The index with every table on the small machine: every batch size,
        // and every pool query as a batch of its own; the others: a size on either side of every threshold, and every fifth pool query.
        for (int v = 0; v < NVARIANTS; ++v) {
            for (int cus : {8, 256}) {
                const bool all = v == OPTPFOR_ALL && cus == 8;
                for (uint32_t nq : all ? ALL_SIZES : cus == 8 ? EDGE_SIZES : FEW_SIZES)
                    for (uint32_t first = 0; first < (nq == 1 || nq == 2 ? npool : 1u); first += (all && nq == 1 ? 1 : 5))
                        for (int op : OPS) run({(Variant)v, cus, 4, op, 10, nq, first, 0, (nq % 3 == 0) ? 3u : 1u, false, false});
            }
            error_cases(pool); // (failed plans in between: the next batch plans on what they left)
        }
        // k beyond one score per lane, and beyond four
        for (Variant v : {OPTPFOR_ALL, OPTPFOR_NONE, OPT, MIXED_SKIP})
            for (int cus : {8, 256})
                for (int op : OPS)
                    for (uint32_t k : {65u, 257u})
                        for (uint32_t nq : {1u, 64u, 512u, 1536u, 4096u}) {
                            if (!ranked(op) || (v != OPTPFOR_ALL && (cus == 256 || nq == 1536)) || (v == MIXED_SKIP && k == 257)) continue;
                            for (uint32_t first = 0; first < (nq == 1 ? npool : 1u); first += 7) run({v, cus, 4, op, k, nq, first, 0, 1, false, false});
                        }
        // the flags
        for (Variant v : {OPTPFOR_ALL, MIXED_SKIP})
            for (int op : OPS)
                for (uint32_t k : {10u, 65u})
                    for (uint32_t nq : {2u, 64u, 1025u}) {
                        if (!ranked(op) && k != 10) continue;
                        run({v, 8, 4, op | DS2I_OP_REFERENCE_ORDER, k, nq, 20, 0, 1, false, false});
                    }
        for (Variant v : {OPTPFOR_ALL, OPT, OPTPFOR_NONE})
            for (int op : OPS)
                for (uint32_t k : {10u, 257u})
                    for (uint32_t nq : {0u, 1u, 64u, 1537u})
                        if (ranked(op)) run({v, nq == 1537 ? 256 : 8, 4, op | DS2I_OP_TOPK_DOCS, k, nq, 19, 0, 2, false, false});
        for (Variant v : {OPTPFOR_ALL, OPTPFOR_NONE, NO_WAND})
            for (int op : {DS2I_OP_AND, DS2I_OP_AND_FREQ, DS2I_OP_OR})
                for (uint32_t nq : {0u, 1u, 64u, 2049u})
                    for (uint32_t first = 0; first < (nq == 1 ? npool : 1u); first += 4) run({v, 8, 4, op, 0, nq, first, 1, 1, false, false});
        for (int op : {DS2I_OP_AND, DS2I_OP_AND_FREQ, DS2I_OP_OR_FREQ})
            for (uint32_t nq : {64u, 4097u}) run({OPTPFOR_ALL, 8, 4, op, 0, nq, 0, 0, 1, true, false});
        for (int op : OPS)
            for (uint32_t k : {10u, 65u, 257u})
                for (uint32_t nq : {64u, 1024u})
                    if (ranked(op)) run({OPTPFOR_ALL, 8, 4, op, k, nq, 0, 0, 1, true, true});
    }
    // past the 32768-record slices of the list streams
    for (int op : OPS) run({OPTPFOR_ALL, 256, 4, op, 10, 36000, 0, 0, 1, false, false});
    run({OPTPFOR_ALL, 256, 4, DS2I_OP_WAND, 65, 36000, 0, 0, 1, false, false});
    run({OPTPFOR_NONE, 8, 4, DS2I_OP_AND, 0, 36000, 0, 0, 4, false, false});
    // one plan whatever the number of planning threads
    for (Variant v : {OPTPFOR_ALL, OPT})
        for (int op : OPS)
            for (uint32_t k : {10u, 65u})
                for (uint32_t nq : {1024u, 1025u, 4096u, 36000u}) {
                    if ((!ranked(op) && k != 10) || (nq == 36000 && (v != OPTPFOR_ALL || k != 10 || (op != DS2I_OP_AND_FREQ && op != DS2I_OP_WAND)))) continue;
                    if (v == OPT && ((op != DS2I_OP_RANKED_AND && op != DS2I_OP_MAXSCORE && op != DS2I_OP_OR) || nq == 1025)) continue;
                    uint64_t d1 = 0;
                    for (unsigned threads : {1u, 3u, 4u, 16u}) {
                        const uint64_t d = run({v, 8, threads, op, k, nq, 0, 0, 1, false, false});
                        if (threads == 1) d1 = d;
                        REQUIRE(d == d1, "the plan depends on the number of planning threads", threads);
                    }
                }
    std::printf("batch_plan: %llu plans hold\n", g_plans);
    return 0;
}
