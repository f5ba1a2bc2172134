// Every operator in the reference's one-document-per-step order (k_daat, k_daat_long)
// (part of kernels.hip -- included inside its anonymous namespace, once per translation unit of the list-count classes; not a
// stand-alone header)
// ------------------------------------------------------------------ document-at-a-time
template <class CX>
DS2I_DEV float score_of(CX& cx, uint32_t s, float norm_len) {
    return __uint_as_float(cx.m(s, M_QW)) * doc_term_weight(cx.freq(s), norm_len);
}

// stable insertion sort of ord[0..n) by key(slot) (== libstdc++ std::sort for n <= 16)
template <class Key>
DS2I_DEV void sort_ord(uint32_t* ord, uint32_t n, Key key) {
    if (lane_id() == 0) {
        for (uint32_t i = 1; i < n; ++i) {
            uint32_t v = ord[i];
            auto kv = key(v);
            uint32_t j = i;
            while (j > 0 && kv < key(ord[j - 1])) { ord[j] = ord[j - 1]; --j; }
            ord[j] = v;
        }
    }
    wave_sync();
}

// One unit of a reference-order operator. The per-list enumerator state (`meta`: M_WORDS dwords per slot, the same
// memory cx.meta points to), the list order `ord` and the maxscore upper bounds `ub` live wherever the caller keeps
// them: LDS for the <=16-term classes (k_daat), a global scratch area for longer queries (k_daat_long).
template <int OP, class TK = RTopK, class CX>
DS2I_DEV void daat_unit(CX& cx, const BatchArgs& a, const uint32_t uid, uint32_t* meta, uint32_t* ord, float* ubs, const uint32_t tmax) {
    const uint32_t lane = lane_id();
    constexpr bool RANKED = OP >= OP_RANKED_AND;
    {
        // a unit of these operators is a doc-id range [blk_begin, blk_end) of the query (whole range when
        // nparts == 1); inside the unit blk_end plays the role of num_docs (the exhaustion sentinel)
        const Unit u = a.units[uid];
        const uint32_t q = u.q;
        const bool whole = u.nparts == 1;
        const uint32_t N = whole ? a.num_docs : u.blk_end;
        cx.num_docs = N;
        const uint32_t t0 = a.q_off[q], nt = a.q_off[q + 1] - t0;
        unsigned long long count = 0, fsum = 0;
        TK tk;
        tk.init(a.k);
        TK_IN_ORDER(tk); // (every traversal below meets the unit's documents in ascending doc-id order: device_enum.hpp, TopKD::in_order)
        if (nt == 0 || nt > tmax) {
            if (lane == 0) { a.out_count[q] = 0; if (a.out_freq_sum) a.out_freq_sum[q] = 0; }
            if (RANKED) store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
            return;
        }
        if (whole) {
            for (uint32_t i = 0; i < nt; ++i) cx.open(i, a.qterms[t0 + i]);
        } else {
            for (uint32_t i = 0; i < nt; ++i) { cx.bind(i, a.qterms[t0 + i]); cx.next_geq(i, u.blk_begin); }
        }
        if (OP == OP_WAND || OP == OP_MAXSCORE) {
            cx.s_bytes += 4ull * nt; // max_term_weight[term]
            if (a.seed_topk && a.seed_len[q] >= a.k) {
                // the ranked_and pass found >= k documents: its k-th score bounds the final k-th score from below.
                // The two operators sum a document's terms in different orders (size- vs docid-sorted lists), so the
                // floor is relaxed by 1e-5 relative -- far above float32 re-association noise, far below any pruning loss
                const float kth = a.seed_topk[(size_t)q * a.k + a.k - 1];
                tk.floor = __uint_as_float(uniform(__float_as_uint(kth * (1.0f - 1.0e-5f))));
            }
        }
        auto norm_len = [&](uint32_t d) {
            cx.s_bytes += 4;
            ++cx.s_scored;
            return __uint_as_float(uniform(__float_as_uint(a.norm_lens[d])));
        };

        if (OP == OP_AND || OP == OP_AND_FREQ || OP == OP_RANKED_AND) {
            // reference traversal, one candidate at a time (queries.hpp:58-84 / 362-387)
            const unsigned long long mbase = a.out_matches ? a.match_off[q] : 0;
            const unsigned long long mcap = a.out_matches ? a.match_off[q + 1] - mbase : 0;
            uint32_t cand = cx.docid(0);
            uint32_t i = 1;
            while (cand < N) {
                for (; i < nt; ++i) {
                    cx.next_geq(i, cand);
                    uint32_t d = cx.docid(i);
                    if (d != cand) { cand = d; i = 0; break; }
                }
                if (i == nt) {
                    if (OP == OP_RANKED_AND) {
                        float nl = norm_len(cand), score = 0.f;
                        for (i = 0; i < nt; ++i) score += score_of(cx, i, nl);
                        TK_INSERT(tk, score, cand);
                    } else {
                        if (a.out_matches && lane == 0 && count < mcap) a.out_matches[mbase + count] = cand;
                        ++count;
                        if (OP == OP_AND_FREQ) for (i = 0; i < nt; ++i) fsum += cx.freq(i);
                    }
                    cx.next(0);
                    cand = cx.docid(0);
                    i = 1;
                }
            }
        } else if (OP == OP_OR || OP == OP_OR_FREQ || OP == OP_RANKED_OR) {
            // queries.hpp:105-127 / 438-462
            uint32_t cur = N;
            for (uint32_t i = 0; i < nt; ++i) { uint32_t d = cx.docid(i); cur = d < cur ? d : cur; }
            while (cur < N) {
                float score = 0.f, nl = 0.f;
                if (OP == OP_RANKED_OR) nl = norm_len(cur);
                uint32_t nxt = N;
                for (uint32_t i = 0; i < nt; ++i) {
                    if (cx.docid(i) == cur) {
                        if (OP == OP_RANKED_OR) score += score_of(cx, i, nl);
                        if (OP == OP_OR_FREQ) fsum += cx.freq(i);
                        cx.next(i);
                    }
                    uint32_t d = cx.docid(i);
                    nxt = d < nxt ? d : nxt;
                }
                if (OP == OP_RANKED_OR) TK_INSERT(tk, score, cur); else ++count;
                cur = nxt;
            }
        } else if (OP == OP_WAND) {
            // queries.hpp:236-305
            if (lane == 0) for (uint32_t i = 0; i < nt; ++i) ord[i] = i;
            wave_sync();
            auto by_docid = [&](uint32_t s) { return meta[s * M_WORDS + M_DOCID]; };
            sort_ord(ord, nt, by_docid);
            for (;;) {
                float upper = 0.f;
                uint32_t pivot = 0;
                bool found = false;
                for (pivot = 0; pivot < nt; ++pivot) {
                    uint32_t s = uniform(ord[pivot]);
                    if (cx.docid(s) == N) break;
                    upper += __uint_as_float(cx.m(s, M_MAXW));
                    if (tk.would_enter(upper)) { found = true; break; }
                }
                if (!found) break;
                const uint32_t pivot_id = cx.docid(uniform(ord[pivot]));
                if (pivot_id == cx.docid(uniform(ord[0]))) {
                    float score = 0.f, nl = norm_len(pivot_id);
                    for (uint32_t j = 0; j < nt; ++j) {
                        uint32_t s = uniform(ord[j]);
                        if (cx.docid(s) != pivot_id) break;
                        score += score_of(cx, s, nl);
                        cx.next(s);
                    }
                    TK_INSERT(tk, score, pivot_id);
                    sort_ord(ord, nt, by_docid);
                } else {
                    uint32_t nl_ = pivot;
                    while (cx.docid(uniform(ord[nl_])) == pivot_id) --nl_;
                    cx.next_geq(uniform(ord[nl_]), pivot_id);
                    if (lane == 0) {
                        for (uint32_t j = nl_ + 1; j < nt; ++j) {
                            uint32_t x = ord[j], y = ord[j - 1];
                            if (meta[x * M_WORDS + M_DOCID] < meta[y * M_WORDS + M_DOCID]) { ord[j] = y; ord[j - 1] = x; }
                            else break;
                        }
                    }
                    wave_sync();
                }
            }
        } else { // OP_MAXSCORE, queries.hpp:514-577
            if (lane == 0) for (uint32_t i = 0; i < nt; ++i) ord[i] = i;
            wave_sync();
            auto by_maxw = [&](uint32_t s) { return __uint_as_float(meta[s * M_WORDS + M_MAXW]); };
            sort_ord(ord, nt, by_maxw);
            if (lane == 0) {
                float acc = 0.f;
                for (uint32_t i = 0; i < nt; ++i) {
                    float mw = __uint_as_float(meta[ord[i] * M_WORDS + M_MAXW]);
                    acc = i ? acc + mw : mw;
                    ubs[i] = acc;
                }
            }
            wave_sync();
            uint32_t non_ess = 0, cur = N;
            // with a seeded floor some lists are non-essential before the first document (the reference only updates
            // this after a successful insert, queries.hpp:568-574 -- same rule, applied to the initial bound)
            while (non_ess < nt && !tk.would_enter(__uint_as_float(uniform(__float_as_uint(ubs[non_ess])))))
                ++non_ess;
            for (uint32_t i = 0; i < nt; ++i) { uint32_t d = cx.docid(i); cur = d < cur ? d : cur; }
            while (non_ess < nt && cur < N) {
                float score = 0.f, nl = norm_len(cur);
                uint32_t nxt = N;
                for (uint32_t i = non_ess; i < nt; ++i) {
                    uint32_t s = uniform(ord[i]);
                    if (cx.docid(s) == cur) {
                        score += score_of(cx, s, nl);
                        cx.next(s);
                    }
                    uint32_t d = cx.docid(s);
                    nxt = d < nxt ? d : nxt;
                }
                for (uint32_t i = non_ess; i-- > 0;) {
                    float ub = __uint_as_float(uniform(__float_as_uint(ubs[i])));
                    if (!tk.would_enter(score + ub)) break;
                    uint32_t s = uniform(ord[i]);
                    cx.next_geq(s, cur);
                    if (cx.docid(s) == cur) score += score_of(cx, s, nl);
                }
                if (TK_INSERT(tk, score, cur)) {
                    while (non_ess < nt && !tk.would_enter(__uint_as_float(uniform(__float_as_uint(ubs[non_ess])))))
                        ++non_ess;
                }
                cur = nxt;
            }
        }
        if (whole) {
            if (lane == 0) {
                a.out_count[q] = RANKED ? tk.n : count;
                if (a.out_freq_sum) a.out_freq_sum[q] = fsum;
            }
            if (RANKED) store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
        } else {
            if (lane == 0) {
                a.unit_count[uid] = RANKED ? tk.n : count;
                a.unit_freq_sum[uid] = fsum;
            }
            if (RANKED) store_topk(a.unit_topk, a.unit_topk_len, a.k, uid, tk DS2I_DOCS_ARG(a.unit_topk_docs));
        }
    }
}

template <int OP, int TMAX, int CODEC_T = -1>
__global__ void __launch_bounds__(64) DS2I_KN(k_daat)(BatchArgs a) {
    __shared__ Lds<TMAX> L;
    CtxT<CODEC_T, MetaLds> cx = make_ctx<CODEC_T, MetaLds>(L, a);
    for (uint32_t tkt = blockIdx.x; tkt < a.nslice; tkt += gridDim.x)
        daat_unit<OP>(cx, a, a.order[tkt], &L.meta[0][0], L.ord(), L.ub(), (uint32_t)TMAX);
    cx.flush_stats(a.stats);
}

// Queries with more than 16 distinct terms (the reference has no limit, queries.hpp:35-86): the same traversals with
// the per-list state -- 128 doc-ids + 128 freqs + M_WORDS dwords per list, the list order and the upper bounds -- in a
// global scratch area of long_stride dwords per unit instead of LDS; only the decoders' staging stays in LDS.
struct LdsLong {
    uint32_t exc[EXC_LDS_DW];
    uint32_t st[STAGE_DW];
};
template <int OP, class TK = RTopK>
__global__ void __launch_bounds__(64) DS2I_KN(k_daat_long)(BatchArgs a) {
    __shared__ LdsLong L;
    CtxT<-1, MetaLds> cx;
    cx.docs = cx.freqs = nullptr;
    cx.meta.p = nullptr;
    cx.exc = L.exc;
    s16_table_init(L.exc);
    cx.win.st = L.st;
    cx.win.gbase = a.arena;
    cx.win.nbytes = 0;
    cx.arena = a.arena;
    cx.bits0 = a.bits0;
    cx.bits1 = a.bits1;
    cx.codec = a.codec;
    cx.num_docs = a.num_docs;
    cx.block_profile = a.block_profile;
    cx.skip = (const uint2*)a.skip;
    cx.init_stats();
    for (uint32_t tkt = blockIdx.x; tkt < a.nslice; tkt += gridDim.x) {
        const uint32_t uid = a.order[tkt];
        const uint32_t q = a.units[uid].q;
        const uint32_t nt = a.q_off[q + 1] - a.q_off[q];
        uint32_t* base = a.long_scratch + (size_t)tkt * a.long_stride;
        cx.docs = base;
        cx.freqs = base + 128u * nt;
        cx.meta.p = base + 256u * nt;
        uint32_t* ord = cx.meta.p + (uint32_t)M_WORDS * nt;
        float* ub = (float*)(ord + nt);
        daat_unit<OP, TK>(cx, a, uid, cx.meta.p, ord, ub, 0xFFFFFFFFu);
    }
    cx.flush_stats(a.stats);
}

// Order-independent score accumulation for the block-synchronous disjunctive kernel. Which of a document's lists are
// essential when it is met -- hence the order its term scores would be added in -- depends on how far the pruning
// threshold has risen, i.e. on the query's split into parts and on timing. Term scores (float32, computed exactly as
// the reference computes them) are therefore summed in fixed point: integer addition is associative, so a
// document's score is the same bits whatever the order, run to run and for wand / maxscore / ranked_or alike. The
// fixed point is RELATIVE to the query: its unit is 2^-62 of the power of two above the query's score bound (the sum of
// its lists' max scores, the same bits in every part of a split query), so the sum of <= 16 terms fits 63 bits and a term
// loses nothing unless it is 2^-38 of the bound -- scores of 1e-6 (terms in most of the documents) are as exact as
// scores of 20. The result differs from the reference's sequential float sum by a few ulps at most (tests hold 1e-5;
// the reference's own ranked test holds 1e-3, test_ranked_queries.cpp:52).
struct FxScale {
    double to_fx, from_fx; // powers of two
    DS2I_DEV void init(float bound) { // bound >= 0, wave-uniform
        const unsigned long long eb = (__float_as_uint(bound) >> 23) & 0xFFu; // bound < 2^(eb - 126)
        to_fx = __longlong_as_double((long long)((1211ull - eb) << 52));       // 2^(62 - (eb - 126))
        from_fx = __longlong_as_double((long long)((835ull + eb) << 52));
    }
    DS2I_DEV unsigned long long of(float term) const { return (unsigned long long)((double)term * to_fx); } // term >= 0
    DS2I_DEV float value(unsigned long long acc) const { return (float)((double)acc * from_fx); }
};
