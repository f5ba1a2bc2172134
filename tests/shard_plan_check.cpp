// Stand-alone check of collection statistics in the batch planner (ds2i_amd/csrc/batch_plan.{hpp,cpp}; its own main, no HIP): the same
// batches planned over a fabricated PlanIndex without and with PlanIndex::stats_df / stats_num_docs -- every operator, k = 10 and 100, a
// batch that holds a query of more than 16 terms and one that does not, an index with every table and a bare one. With statistics every
// q_weight must be bm25::query_term_weight(qtf, df[term], N) and every product of it must follow from it as the planner forms it; without
// them it is the list's own length and the index's own number of documents; and everything in a plan that is not a product of q_weight
// must be the same in both: the route, the terms and their order, the classes, and -- but for the union streams -- the units, the launch
// groups and the layout. (The union streams order a query's driving lists by their bounds and leave out the lists whose bounds lie below
// the query's static floor: both are products of q_weight, so there the units follow from it as well.)
// Built with -fsanitize=address,undefined by tests/test_shard_abi_cpu.py. Prints "shard_plan: N plans hold" and returns 0, or says what
// differs and returns 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../ds2i_amd/csrc/batch_plan.hpp"
#include "../ds2i_amd/csrc/host_index.hpp"

using ds2i_dev::QTerm;
using ds2i_dev::Unit;
using ds2i_host::bm25;

static const uint32_t NUM_DOCS = 1u << 17;
static const uint64_t COLLECTION_DOCS = 3ull * NUM_DOCS + 11;
static const uint32_t NLISTS = 24;
static const uint32_t LIST_SIZES[NLISTS] = {3, 17, 40, 64, 127, 128, 129, 200, 300, 513, 650, 777, 900, 2047, 2048, 2300, 2700, 3100, 3600, 4096,
                                            23000, 34000, 46000, 58000};

static std::string g_where;
#define REQUIRE(cond, what)                                                            \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("shard_plan: %s: %s (%s)\n", g_where.c_str(), what, #cond);    \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

struct Fab {
    std::vector<QTerm> proto;
    std::vector<uint32_t> n, df;
    std::vector<float> topbmw;
    Ds2iKnobs knobs;
    PlanIndex ix;
};

static void fabricate(Fab& f, bool tables) {
    f.proto.assign(NLISTS, QTerm{});
    f.n.assign(NLISTS, 0);
    f.df.assign(NLISTS, 0);
    f.topbmw.assign((size_t)NLISTS * DS2I_HIP_MAX_K, 0.f);
    uint64_t off = 0, blk = 0, tail = 0, rmw64 = 0;
    for (uint32_t t = 0; t < NLISTS; ++t) {
        const uint32_t n = LIST_SIZES[t], nb = (n + 127) / 128;
        QTerm& q = f.proto[t];
        q.list_off = off;
        off += 5 + 3 * (uint64_t)n;
        q.list_end = off;
        q.n = n;
        q.q_weight = 0.5f + 0.015625f * (float)t;          // (parked: max_term_weight)
        q.max_weight = 0.875f - 0.0078125f * (float)(t % 7); // (parked: the list's largest block weight)
        q.term = t;
        q.aux0 = blk;
        q.aux1 = tail;
        q.blk_base = (uint32_t)blk;
        uint32_t shift = 0;
        while (shift < 31 && ((uint64_t)NUM_DOCS >> (shift + 1)) >= 4ull * n) ++shift;
        q.rmw_off64 = (uint32_t)rmw64;
        q.rmw_shift = shift;
        q.nblocks = nb;
        rmw64 += (ds2i_dev::RmwLevels(NUM_DOCS, shift).bytes() + ds2i_dev::RmwLevels::bitmap_bytes(NUM_DOCS)) / 64;
        blk += nb;
        tail += n % 128;
        f.n[t] = n;
        // the collection holds more of every term, and not in proportion: the idf order of the terms is not the shard's
        f.df[t] = n + (t % 2 ? 5 * n : n / 3) + t;
        for (uint32_t j = 0; j < DS2I_HIP_MAX_K && j < nb; ++j) f.topbmw[(size_t)t * DS2I_HIP_MAX_K + j] = q.max_weight * (1.0f - (float)j / 128.0f);
    }
    std::memset(&f.knobs, 0, sizeof f.knobs);
    f.knobs.rmw_g = 4.0;
    f.knobs.ut_blocks = 320;
    f.knobs.stream_nt_max = 16;
    f.knobs.plan_threads = 3;
    PlanIndex& ix = f.ix;
    ix = PlanIndex{};
    ix.kind = DS2I_BLOCK_OPTPFOR;
    ix.num_cus = 256;
    ix.size = NLISTS;
    ix.num_docs = NUM_DOCS;
    ix.has_wand = true;
    ix.skip = tables;
    ix.bmw = ix.rmw = ix.has_bitmaps = ix.side_tables = ix.bound_tables = tables;
    ix.skip_or_pef = ix.skip;
    ix.knobs = &f.knobs;
    ix.term_proto = f.proto.data();
    ix.list_n = f.n.data();
    ix.list_topbmw = f.topbmw.data();
}

typedef std::vector<uint32_t> Query;

static std::vector<Query> queries(bool with_long) {
    std::vector<Query> qs;
    qs.push_back({});
    for (uint32_t n = 1; n <= 16; ++n) {
        Query q;
        for (uint32_t i = 0; i < n; ++i) q.push_back((5 * n + 7 * i) % NLISTS);
        qs.push_back(q);
    }
    for (Query q : {Query{5, 5}, Query{3, 9, 3}, Query{20, 13, 20, 13}, Query{14, 15}, Query{20, 21}, Query{22, 23}, Query{20, 21, 22, 23}, Query{23},
                    Query{0, 14}, Query{13, 20, 21, 22, 23, 18}})
        qs.push_back(q);
    if (with_long) {
        Query q20;
        for (uint32_t t = 2; t < 22; ++t) q20.push_back(t); // 20 distinct terms, one of them twice
        q20.push_back(7);
        qs.push_back(q20);
    }
    std::vector<Query> batch;
    for (uint32_t i = 0; i < 300; ++i) batch.push_back(qs[(i * 7) % qs.size()]);
    return batch;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// what is no product of q_weight in a term record
static std::tuple<uint64_t, uint64_t, uint32_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t> fixed_part(const QTerm& t) {
    return std::make_tuple(t.list_off, t.list_end, t.n, t.term, t.aux0, t.aux1, t.blk_base, t.rmw_off64, t.rmw_shift, t.nblocks);
}

static void check_weights(const BatchPlan& b, const Fab& f, const std::vector<Query>& batch, bool stats) {
    const bool us = b.route.union_stream;
    const std::vector<QTerm>& real = us ? b.vterms : b.qterms;
    const std::vector<uint32_t>& roff = us ? b.voff : b.qoff;
    REQUIRE(roff.size() == batch.size() + 1, "query offsets");
    std::vector<std::map<uint32_t, uint32_t>> qtf(batch.size());
    for (size_t q = 0; q < batch.size(); ++q)
        for (uint32_t t : batch[q]) ++qtf[q][t];
    auto check_term = [&](const QTerm& t, size_t q) {
        REQUIRE(t.term < NLISTS && qtf[q].count(t.term), "a term of another query");
        const float own = bm25::query_term_weight(qtf[q][t.term], f.n[t.term], NUM_DOCS);
        const float coll = bm25::query_term_weight(qtf[q][t.term], f.df[t.term], COLLECTION_DOCS);
        if (!b.route.ranked) {
            REQUIRE(t.q_weight == 0.f && t.max_weight == 0.f, "weights of an unranked operator");
            return;
        }
        REQUIRE(same_bits(t.q_weight, stats ? coll : own), stats ? "q_weight is not query_term_weight(qtf, df, N)" : "q_weight without statistics");
        const float lbmw = f.proto[t.term].max_weight;
        if (f.ix.bmw) REQUIRE(same_bits(t.max_bmw, t.q_weight * lbmw), "max_bmw does not follow from q_weight");
        REQUIRE(same_bits(t.rmw_scale, t.q_weight * (lbmw * (1.0f / 255.0f))), "rmw_scale does not follow from q_weight");
    };
    for (size_t q = 0; q < batch.size(); ++q) {
        REQUIRE(roff[q + 1] - roff[q] == qtf[q].size(), "distinct terms of a query");
        for (uint32_t i = roff[q]; i < roff[q + 1]; ++i) {
            check_term(real[i], q);
            if (!us && b.route.ranked) REQUIRE(same_bits(real[i].max_weight, real[i].q_weight * f.proto[real[i].term].q_weight), "max_weight does not follow from q_weight");
        }
    }
    if (us)
        for (size_t v = 0; v + 1 < b.qoff.size(); ++v)
            for (uint32_t i = b.qoff[v]; i < b.qoff[v + 1]; ++i) check_term(b.qterms[i], b.vinfo[3 * v]);
}

// The units of a union-stream plan against the weights the plan itself holds (cut_union_query restated): a query's lists by decreasing
// bound (stable), S_e = the bounds from e down, list e drives a virtual query unless e > 0 and S_e lies below the query's static floor;
// the virtual queries come in that order, each with all of the query's lists, and the units of each cover its driving list's blocks.
// With statistics the bounds are other numbers, so the units may be others: they must be the ones these weights give.
static void check_union_units(const BatchPlan& b) {
    REQUIRE(b.route.union_stream && b.q_unit_off.size() == (size_t)b.nq + 1 && b.vinfo.size() == 3 * (b.qoff.size() - 1), "the shape of a union-stream plan");
    for (uint32_t q = 0; q < b.nq; ++q) {
        const uint32_t u0 = b.q_unit_off[q], u1 = b.q_unit_off[q + 1], begin = b.voff[q], nt = b.voff[q + 1] - begin;
        if (u0 == u1) continue; // a one-term query the seed pass answers
        if (nt == 0) {          // the empty query: one unit of an empty virtual query
            const uint32_t v = b.units[u0].q;
            REQUIRE(u1 - u0 == 1 && (size_t)v + 1 < b.qoff.size() && b.qoff[v + 1] == b.qoff[v] && b.vinfo[3 * (size_t)v] == q, "the unit of the empty query");
            continue;
        }
        REQUIRE(nt >= 1 && nt <= DS2I_HIP_MAX_TERMS, "units of a query the streams do not take");
        uint32_t ord[DS2I_HIP_MAX_TERMS];
        for (uint32_t i = 0; i < nt; ++i) ord[i] = i;
        for (uint32_t i = 1; i < nt; ++i) {
            const uint32_t v = ord[i];
            uint32_t j = i;
            while (j > 0 && b.vterms[begin + v].max_bmw > b.vterms[begin + ord[j - 1]].max_bmw) { ord[j] = ord[j - 1]; --j; }
            ord[j] = v;
        }
        float suffix[DS2I_HIP_MAX_TERMS + 1];
        suffix[nt] = 0.f;
        for (uint32_t e = nt; e-- > 0;) suffix[e] = suffix[e + 1] + b.vterms[begin + ord[e]].max_bmw;
        const float f1 = b.vterms[begin].floor1;
        uint32_t u = u0;
        for (uint32_t e = 0; e < nt; ++e) {
            if (e && suffix[e] * (1.0f + 1.0f / 65536.0f) < f1 * (1.0f - 1.0e-5f)) break;
            REQUIRE(u < u1, "a driving list without units");
            const uint32_t v = b.units[u].q;
            REQUIRE((size_t)v + 1 < b.qoff.size() && b.vinfo[3 * (size_t)v] == q && b.vinfo[3 * (size_t)v + 1] == e, "the virtual queries of a query, in order");
            REQUIRE(b.qoff[v + 1] - b.qoff[v] == nt, "a virtual query holds all lists of its query");
            const QTerm& drv = b.qterms[b.qoff[v]];
            REQUIRE(fixed_part(drv) == fixed_part(b.vterms[begin + ord[e]]), "the driving list of a virtual query");
            REQUIRE(same_bits(drv.suf_bmw, suffix[e + 1]) && same_bits(drv.max_weight, suffix[0]) && same_bits(drv.floor1, f1), "the bounds of a driving list");
            const uint32_t nbe = std::max(1u, drv.nblocks);
            uint32_t at = 0;
            while (u < u1 && b.units[u].q == v) {
                REQUIRE(b.units[u].blk_begin == at && b.units[u].blk_end > at && b.units[u].nparts == u1 - u0, "a unit of a virtual query");
                at = b.units[u].blk_end;
                ++u;
            }
            REQUIRE(at == nbe, "the units of a virtual query do not cover its driving list");
        }
        REQUIRE(u == u1, "units beyond the driving lists the weights give");
    }
}

static void compare(const BatchPlan& a, const BatchPlan& b) {
    const Route &x = a.route, &y = b.route;
    REQUIRE(x.base_op == y.base_op && x.conj == y.conj && x.ranked == y.ranked && x.reference == y.reference && x.disj_topk == y.disj_topk &&
            x.bigk == y.bigk && x.bigk_stream == y.bigk_stream && x.bigk_union == y.bigk_union && x.stream_nt_max == y.stream_nt_max &&
            x.union_stream == y.union_stream && x.us_ok == y.us_ok && x.list_stream == y.list_stream && x.and_stream == y.and_stream &&
            x.and_rs_units == y.and_rs_units && x.freq_stream == y.freq_stream && x.rs_ok == y.rs_ok && x.rs_nt == y.rs_nt &&
            x.rs_classes == y.rs_classes && x.exact == y.exact && x.seeded == y.seeded && x.docs == y.docs, "the route");
    REQUIRE(a.op == b.op && a.k == b.k && a.nq == b.nq && a.use_seed == b.use_seed && a.hist == b.hist, "the plan's header");
    REQUIRE(a.seed_terms == b.seed_terms && a.seed_offs == b.seed_offs && a.qnb0 == b.qnb0, "seed terms");
    for (int c = 0; c < NCLS; ++c) REQUIRE(a.nqcls[c] == b.nqcls[c], "the queries of a class");
    {
        const std::vector<QTerm>& ra = x.union_stream ? a.vterms : a.qterms;
        const std::vector<QTerm>& rb = y.union_stream ? b.vterms : b.qterms;
        const std::vector<uint32_t>& oa = x.union_stream ? a.voff : a.qoff;
        REQUIRE(ra.size() == rb.size() && oa == (y.union_stream ? b.voff : b.qoff), "the terms of the queries");
        for (size_t i = 0; i < ra.size(); ++i) REQUIRE(fixed_part(ra[i]) == fixed_part(rb[i]), "the order of a query's terms");
    }
    // The union streams drive a query by its lists in the order of their bounds and give no units to the lists whose bounds lie below the
    // query's static floor (cut_union_query): bounds and floor are products of q_weight, so units, groups and layout follow from it there.
    // What is held instead: each plan's units are the ones its own weights give (check_union_units).
    if (x.union_stream) {
        check_union_units(a);
        check_union_units(b);
        return;
    }
    REQUIRE(a.nunits == b.nunits && a.nsplit == b.nsplit && a.nsingle == b.nsingle && a.long_terms == b.long_terms, "the counts");
    REQUIRE(a.qoff == b.qoff && a.voff == b.voff && a.q_unit_off == b.q_unit_off && a.qnb0 == b.qnb0, "offsets");
    REQUIRE(a.split_queries == b.split_queries && a.single_queries == b.single_queries && a.empty_queries == b.empty_queries, "query lists");
    REQUIRE(a.seed_terms == b.seed_terms && a.seed_offs == b.seed_offs && a.match_off == b.match_off, "seed terms");
    REQUIRE(a.up_bytes == b.up_bytes && a.out_bytes == b.out_bytes && a.scr_bytes == b.scr_bytes && a.o_qterms == b.o_qterms && a.o_units == b.o_units &&
            a.o_topk == b.o_topk && a.o_topk_docs == b.o_topk_docs, "the layout");
    for (int c = 0; c < NCLS; ++c) {
        REQUIRE(a.ncls[c] == b.ncls[c] && a.nqcls[c] == b.nqcls[c], "the classes");
        REQUIRE(a.sub[c].size() == b.sub[c].size(), "launch groups of a class");
        for (size_t g = 0; g < a.sub[c].size(); ++g)
            REQUIRE(a.sub[c][g].end - a.sub[c][g].begin == b.sub[c][g].end - b.sub[c][g].begin && a.sub[c][g].lists == b.sub[c][g].lists &&
                    a.sub[c][g].kernel == b.sub[c][g].kernel, "a launch group");
    }
    REQUIRE(a.units.size() == b.units.size() && a.sterms.size() == b.sterms.size(), "sizes");
    for (size_t u = 0; u < a.units.size(); ++u) REQUIRE(std::memcmp(&a.units[u], &b.units[u], sizeof(Unit)) == 0, "a unit");
    for (int c = 0; c < NCLS; ++c) REQUIRE(a.cls_units[c] == b.cls_units[c] && a.order[c] == b.order[c], "units of a class and their order");
    for (size_t i = 0; i < a.sterms.size(); ++i) REQUIRE(std::memcmp(&a.sterms[i], &b.sterms[i], sizeof a.sterms[i]) == 0, "a list-stream record");
}

int main() {
    unsigned long long plans = 0;
    static const int OPS[] = {DS2I_OP_AND, DS2I_OP_AND_FREQ, DS2I_OP_OR, DS2I_OP_OR_FREQ, DS2I_OP_RANKED_AND, DS2I_OP_WAND, DS2I_OP_MAXSCORE, DS2I_OP_RANKED_OR,
                              DS2I_OP_RANKED_AND | DS2I_OP_TOPK_DOCS, DS2I_OP_WAND | DS2I_OP_TOPK_DOCS};
    bool weights_differ = false;
    for (int tables = 0; tables < 2; ++tables)
        for (int with_long = 0; with_long < 2; ++with_long) {
            Fab f;
            fabricate(f, tables != 0);
            const std::vector<Query> batch = queries(with_long != 0);
            std::vector<uint32_t> terms, offs(1, 0);
            for (const Query& q : batch) {
                terms.insert(terms.end(), q.begin(), q.end());
                offs.push_back((uint32_t)terms.size());
            }
            for (int op : OPS)
                for (uint32_t k : {10u, 100u}) {
                    g_where = "op " + std::to_string(op) + ", k " + std::to_string(k) + (tables ? ", tables" : ", bare") + (with_long ? ", a long query" : "");
                    PlanRequest rq;
                    rq.op = op;
                    rq.k = k;
                    rq.terms = terms.data();
                    rq.query_offsets = offs.data();
                    rq.nq = (uint32_t)batch.size();
                    BatchPlan plain, with, seed_plain, seed_with, again;
                    PlanIndex ix = f.ix;
                    REQUIRE(plan_batch(plain, ix, rq) == DS2I_OK, "the batch does not plan");
                    ix.stats_num_docs = COLLECTION_DOCS;
                    ix.stats_df = f.df.data();
                    REQUIRE(plan_batch(with, ix, rq) == DS2I_OK, "the batch does not plan with statistics");
                    check_weights(plain, f, batch, false);
                    check_weights(with, f, batch, true);
                    compare(plain, with);
                    if (plain.use_seed) { // the ranked_and pass ahead of wand / maxscore / ranked_or: planned like any other batch
                        REQUIRE(plan_batch(seed_plain, f.ix, seed_request(plain)) == DS2I_OK && plan_batch(seed_with, ix, seed_request(with)) == DS2I_OK,
                                "the seed pass does not plan");
                        compare(seed_plain, seed_with);
                        plans += 2;
                    }
                    // cleared again: the plan is the first one's, weights and all
                    REQUIRE(plan_batch(again, f.ix, rq) == DS2I_OK, "the batch does not plan once the statistics are cleared");
                    check_weights(again, f, batch, false);
                    if (plain.route.ranked && !plain.route.union_stream) // (the union streams' virtual queries need not pair up)
                        for (size_t i = 0; i < plain.qterms.size() && i < with.qterms.size(); ++i) weights_differ = weights_differ || !same_bits(plain.qterms[i].q_weight, with.qterms[i].q_weight);
                    plans += 3;
                }
        }
    g_where = "all";
    REQUIRE(weights_differ, "the statistics changed no weight");
    std::printf("shard_plan: %llu plans hold\n", plans);
    return 0;
}
