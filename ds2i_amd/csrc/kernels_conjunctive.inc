// and_query / ranked_and_query as block-synchronous class kernels (k_conjunctive) + k_merge
// (part of kernels.hip -- included inside its anonymous namespace, once per translation unit of the list-count classes; not a
// stand-alone header)
// ------------------------------------------------------------------ conjunctive
// Candidate membership of c (held by this lane, valid iff `want`) in the sorted LDS block d[128].
DS2I_DEV bool member_bsearch(const uint32_t* d, uint32_t c, bool want, uint32_t& pos) {
    uint32_t idx = 0;
    if (want) {
#pragma unroll
        for (uint32_t step = 64; step; step >>= 1)
            if (d[idx + step - 1] < c) idx += step;
    }
    pos = idx;
    return want && d[idx] == c;
}

// Runs body(i) for i in [FROM, nt); body returns false to break. With REG the loop is expanded at compile time
// (template recursion), so i is a constant inside the body and the register-resident enumerator state is never
// indexed dynamically; otherwise it is a plain loop.
template <int I, int N, class F>
DS2I_DEV bool static_list_loop(uint32_t nt, F& f) {
    if constexpr (I < N) {
        if ((uint32_t)I >= nt) return true;
        if (!f(std::integral_constant<uint32_t, (uint32_t)I>{})) return false;
        return static_list_loop<I + 1, N>(nt, f);
    }
    return true;
}
// body(integral_constant i) for i = HI-1 down to LO, compile-time expanded
template <int HI, int LO, class F>
DS2I_DEV void static_loop_down(F& f) {
    if constexpr (HI > LO) {
        f(std::integral_constant<uint32_t, (uint32_t)(HI - 1)>{});
        static_loop_down<HI - 1, LO>(f);
    }
}
#define DS2I_LIST_LOOP(FROM, body)                                   \
    if constexpr (REG) {                                             \
        static_list_loop<(FROM), TMAX>(nt, body);                    \
    } else {                                                         \
        for (uint32_t i_ = (FROM); i_ < nt; ++i_)                    \
            if (!body(i_)) break;                                    \
    }

// Waves per SIMD the conjunctive kernels are compiled for. <=2 lists: 6 (80 VGPRs, 12 B/lane of scratch; measured on the
// GOV2-scale batch: 6 / 7 / 8 waves = 210 / 209 / 203 k queries/s -- the spills of the tighter budgets cost what the
// extra waves hide); beyond that LDS caps the residency anyway (8 / 13 / 23 KiB per wave of the 160 KiB per CU), and
// without a bound the register allocator lets the unrolled list loops balloon (237 VGPRs, 2 waves/SIMD for the 4-list
// kernel when left alone).
#ifndef DS2I_FLOOR_EVERY
#define DS2I_FLOOR_EVERY 4 // power of two
#endif
static_assert(DS2I_FLOOR_EVERY > 0 && (DS2I_FLOOR_EVERY & (DS2I_FLOOR_EVERY - 1)) == 0, "DS2I_FLOOR_EVERY is used as a mask: power of two");
#ifndef DS2I_OCC2
#define DS2I_OCC2 6
#endif
#define CONJ_WAVES(T) ((T) <= 2 ? DS2I_OCC2 : (T) <= 4 ? 5 : (T) <= 8 ? 3 : 1)
// and / and_freq carry no scoring state: their <=2-list kernels fit 8 waves/SIMD (59-61 VGPRs, no scratch)
#define CONJ_WAVES_R(RANKED, T) (!(RANKED) && (T) <= 2 ? 8 : CONJ_WAVES(T))

// LDS of the conjunctive kernels: the shared layout plus, for ranked_and, the norm_len of every posting of list 0's
// current block (-1 = the posting was dropped by the freq-only bound and its norm_len never fetched) and its list-0 term
// score; ranked_and has no use for the match positions (it scores progressively). 5540 B for <=2 lists: 29 waves per
// CU fit, 24 (6 per SIMD) are used.
template <int TMAX, bool META_IN_LDS, bool RANKED, bool WITH_S16 = true>
struct LdsConj : Lds<TMAX, META_IN_LDS, !RANKED, WITH_S16, (RANKED && TMAX > 2) ? 2 : TMAX> {
    float nl[RANKED ? 128 : 1];
    float part0[RANKED ? 128 : 1]; // list-0 term score of each posting of the block (-inf = dropped): read every round
    // range-table bytes of each posting of list 0's block in the other lists, packed: byte i-1 of qb = list i (1..4),
    // byte i-5 of qb2 = list i (5..7)
    uint32_t qb[RANKED ? 128 : 1];
    uint32_t qb2[RANKED && (TMAX > 4) ? 128 : 1];
};

template <bool RANKED, bool WITH_FREQS, int TMAX, int CODEC_T, bool STATS = true>
__global__ void __launch_bounds__(64, CONJ_WAVES_R(RANKED, TMAX)) DS2I_KN(k_conjunctive)(BatchArgs a) {
    // <=4 lists: every list loop below is fully unrolled, so the enumerator state is addressed with constants
    // and lives in registers (MetaReg); 8/16 lists keep it in LDS (code size)
    constexpr bool REG = TMAX <= 4;
    typedef typename std::conditional<REG, MetaReg<TMAX>, MetaLds>::type META;
    __shared__ LdsConj<TMAX, !REG, RANKED, CODEC_T != CODEC_PEF && CODEC_T != CODEC_OPTPFOR> L; // (no Simple16 field table for the Elias-Fano layouts and for block_optpfor through its side slots)
    const uint32_t lane = lane_id();
    // ranked_and with 3+ lists: one freqs buffer for list 0, one shared by the others (each is used where it is decoded)
    constexpr bool SHARE_F = RANKED && TMAX > 2;
    CtxT<CODEC_T, META, STATS, SHARE_F> cx = make_ctx<CODEC_T, META, STATS, SHARE_F>(L, a);
    cx.want_freqs = WITH_FREQS && !RANKED; // and_freq reads the freq of every match: both parts of a block in one pass (side slots)
    // ranked_and only: per-block max doc_term_weight table (null = no pruning). Three levels, all exact (the bounds
    // are true upper bounds of the float32 score and topk_queue::insert is strict, queries.hpp:157-172):
    //   * blocks of list 0 whose bound cannot enter the heap are skipped without being decoded (skip_list0);
    //   * SCORE-FIRST rounds, once the heap is full or a floor is known: the list-0 term score of every candidate is
    //     computed first; a candidate goes on to list i only while its partial score + the later lists' list maxima can
    //     still enter the heap, so the long lists are probed -- and their blocks decoded -- for few candidates;
    //   * before list i's next block is decoded, the best alive partial score + that block's max weight is tested.
    const float* const bmw = RANKED ? a.bmw : nullptr;
    // Doc-id-range tables (BatchArgs::rmw): one byte gather per candidate and other list, no search. A zero byte proves
    // the candidate is in no intersection with that list; otherwise the bytes bound its score in the other lists far
    // tighter than the list maxima (M_SUF) do. Lists 1..7 of a query are covered (the 9-16-term class keeps M_SUF).
    constexpr int RL = TMAX < 8 ? TMAX : 8; // lists 1 .. RL-1 have their bytes packed per candidate
    const uint8_t* const rmw = TMAX <= 8 ? a.rmw : nullptr;
    // one work unit per (single-wave) workgroup, costliest units first: the hardware dispatcher
    // interleaves the workgroups of the concurrently running LDS classes as resources free up
    for (uint32_t tkt = blockIdx.x; tkt < a.nslice; tkt += gridDim.x) {
        const uint32_t uid = a.order[tkt];
        const unsigned long long t_unit = (STATS && a.unit_clock) ? wall_clock64() : 0ull;
        const Unit u = a.units[uid];
#ifdef DS2I_PHASE_TIMING
        const unsigned long long unit_t0 = __builtin_readcyclecounter();
#endif
        const uint32_t q = u.q;
        const bool whole = u.nparts == 1;
        const uint32_t t0 = a.q_off[q], nt = a.q_off[q + 1] - t0;
        unsigned long long count = 0, fsum = 0;
        RTopK tk;
        tk.init(a.k);
        if (nt == 0 || nt > (uint32_t)TMAX) { // empty query -> 0 results (queries.hpp:41,335)
            if (lane == 0) { a.out_count[q] = 0; if (a.out_freq_sum) a.out_freq_sum[q] = 0; }
            if (RANKED) store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
            continue;
        }
        // list 0 (shortest) drives; the unit owns its blocks [blk_begin, blk_end). The other lists are
        // bound lazily: their first block is located by the first candidate (no block-0 decode).
        auto bind_one = [&](auto ic) __attribute__((always_inline)) { const uint32_t i = ic; cx.bind(i, a.qterms[t0 + i]); return true; };
        DS2I_LIST_LOOP(0, bind_one)
        const unsigned long long mbase = a.out_matches ? a.match_off[q] + 128ull * u.blk_begin : 0;
        const unsigned long long mcap = a.out_matches ? 128ull * (u.blk_end - u.blk_begin) : 0;
        // ---- pruning state (ranked_and with a bmw table)
        // the parts of a split query share a score histogram (ScoreHist): the floor it yields is exact to compare against,
        // since all parts add a document's terms in the same order (a dropped document scores <= floor <= final threshold)
        const bool shared_floor = RANKED && bmw && !whole && a.q_hist;
        ScoreHist sh;
        sh.init(shared_floor ? a.q_hist : nullptr, shared_floor ? a.q_hist_slot[q] : 0u,
                shared_floor ? __uint_as_float(uniform(__float_as_uint(a.qterms[t0].max_bmw + a.qterms[t0].suf_bmw))) : 0.f,
                1.0f - 1.0f / 1048576.0f);
        auto adopt_floor = [&]() __attribute__((always_inline)) {
            const float f = sh.floor(tk.k);
            if (f > tk.floor) tk.floor = f;
        };
        if (RANKED && bmw && nt == 1) // k blocks of the list hold a document reaching floor1 (computed at upload)
            tk.floor = __uint_as_float(uniform(__float_as_uint(a.qterms[t0].floor1)));
        if (shared_floor) adopt_floor();
        auto can_prune = [&]() { return tk.n >= tk.k || tk.floor > 0.f; };
        const float* const w0tab = bmw ? bmw + cx.m(0, M_PBASE) : nullptr;
        // first block >= blk of list 0, inside the unit, whose bound (its own max weight + the other lists' list maxima)
        // can enter the heap: 64 table entries per probe, nothing decoded
        auto skip_list0 = [&](uint32_t blk) __attribute__((always_inline)) -> uint32_t {
            if (!RANKED || !bmw || !can_prune()) return blk;
            const float qw0 = __uint_as_float(cx.m(0, M_QW)), suf0 = __uint_as_float(cx.m(0, M_SUF));
            while (blk < u.blk_end) {
                const uint32_t idx = blk + lane;
                float w = 0.f;
                if (idx < u.blk_end) w = w0tab[idx];
                const float ub = (qw0 * w + suf0) * BOUND_SLACK;
                const uint64_t hit = ballot(idx < u.blk_end && tk.would_enter(ub));
                if (hit) return blk + (uint32_t)__builtin_ctzll(hit);
                blk += 64;
            }
            return u.blk_end;
        };
        const bool use_rmw = rmw && nt > 1 && (!RANKED || bmw); // wave-uniform
        // the range-table bytes of candidate c in lists 1..nt-1 (all gathers are issued before the first is consumed);
        // false = some list has no posting in c's range, so c cannot be a match
        auto rmw_gather = [&](uint32_t c, bool valid, uint32_t& qlo, uint32_t& qhi) __attribute__((always_inline)) -> bool {
            uint32_t e[RL] = {};
            auto load_one = [&](auto ic) __attribute__((always_inline)) {
                constexpr uint32_t i = decltype(ic)::value;
                const uint8_t* tab = rmw + 64ull * cx.m(i, M_RBASE);
                e[i] = valid ? (uint32_t)tab[c >> cx.m(i, M_RSHIFT)] : 0u;
                return true;
            };
            // two trips: list 1 first, the other lists only for the candidates inside list 1's ranges (a table holds 4..8
            // entries per posting, so a random document is outside with probability ~0.85 whatever the list's length).
            // A gather is one cache-line request per lane, and with 3+ lists the L1's request rate, not the latency, was
            // what the gathers cost: 500 k -> 525 k queries/s on the GOV2-scale batch.
            load_one(std::integral_constant<uint32_t, 1>{});
            valid = valid && e[1] != 0;
            static_list_loop<2, RL>(nt, load_one);
            bool ok = valid;
            qlo = qhi = 0;
            auto pack_one = [&](auto ic) __attribute__((always_inline)) {
                constexpr uint32_t i = decltype(ic)::value;
                ok = ok && e[i] != 0;
                if constexpr (i <= 4) qlo |= e[i] << (8 * (i - 1)); else qhi |= e[i] << (8 * (i - 5));
                return true;
            };
            static_list_loop<1, RL>(nt, pack_one);
            return ok;
        };
        // bound of the candidate's term score in list i, from its packed byte
        auto rmw_term = [&](uint32_t qlo, uint32_t qhi, auto ic) __attribute__((always_inline)) -> float {
            constexpr uint32_t i = decltype(ic)::value;
            const uint32_t b = i <= 4 ? (qlo >> (8 * (i - 1))) & 255u : (qhi >> (8 * ((i - 5) & 3))) & 255u;
            return __uint_as_float(cx.m(i, M_RSCALE)) * (float)b;
        };
        // sum of those bounds over the lists j > after (added from the last list down, so that the value for `after` is a
        // prefix of the same chain whatever `after` is)
        auto rmw_rest = [&](uint32_t qlo, uint32_t qhi, uint32_t after) __attribute__((always_inline)) -> float {
            float r = 0.f;
            auto add_one = [&](auto jc) __attribute__((always_inline)) {
                constexpr uint32_t j = decltype(jc)::value;
                if (j < nt && j > after) r = r + rmw_term(qlo, qhi, jc);
            };
            static_loop_down<RL, 1>(add_one);
            return r;
        };
        // and_query only: lists dense enough to carry an exact bitmap (bit i of bm_lists) are tested by a bit gather and then
        // never probed or decoded -- membership is all and_query wants from them; the others go by their range-table byte
        // (zero = not a member for sure) and are verified by the usual probe
        uint32_t bm_lists = 0;
        if constexpr (!RANKED) { // (and_freq filters by the bitmap too -- exact, where a byte covering 1..4 doc-ids of a dense list
                                 // mostly is not zero -- but still probes the list: it needs the matching postings' freqs)
            if (use_rmw && a.rmw_bitmaps) {
                auto mark = [&](auto ic) __attribute__((always_inline)) {
                    constexpr uint32_t i = decltype(ic)::value;
                    if (RmwLevels::has_bitmap(cx.m(i, M_N), a.num_docs)) bm_lists |= 1u << i;
                    return true;
                };
                static_list_loop<1, RL>(nt, mark);
            }
        }
        auto and_filter = [&](uint32_t c, bool valid) __attribute__((always_inline)) -> bool {
            uint32_t e[RL] = {};
            auto load_one = [&](auto ic) __attribute__((always_inline)) {
                constexpr uint32_t i = decltype(ic)::value;
                const uint8_t* tab = rmw + 64ull * cx.m(i, M_RBASE);
                if ((bm_lists >> i) & 1u) {
                    const uint32_t* bm = (const uint32_t*)(tab + RmwLevels(a.num_docs, cx.m(i, M_RSHIFT)).bytes());
                    e[i] = valid ? (bm[c >> 5] >> (c & 31u)) & 1u : 0u;
                } else {
                    e[i] = valid ? (uint32_t)tab[c >> cx.m(i, M_RSHIFT)] : 0u;
                }
                return true;
            };
            static_list_loop<1, RL>(nt, load_one);
            bool ok = valid;
            auto test_one = [&](auto ic) __attribute__((always_inline)) { ok = ok && e[decltype(ic)::value] != 0; return true; };
            static_list_loop<1, RL>(nt, test_one);
            if (a.rmh && ballot(ok)) {
                // membership hints (BatchArgs::rmh; block_optpfor indexes): for the candidates every list's byte lets through, the
                // lists without a bitmap say WHICH document of the candidate's range is theirs (where it is the only one): a
                // candidate elsewhere in that range is not a member and is never probed. All hint loads first, then the tests.
                const long long hd = (long long)(a.rmh - a.rmw);
                uint32_t h[RL] = {};
                auto load_hint = [&](auto ic) __attribute__((always_inline)) {
                    constexpr uint32_t i = decltype(ic)::value;
                    h[i] = 255u;
                    if (!((bm_lists >> i) & 1u)) {
                        const uint8_t* ht = rmw + 64ull * cx.m(i, M_RBASE) + hd;
                        if (ok && cx.m(i, M_RSHIFT) != 0u) h[i] = (uint32_t)ht[c >> cx.m(i, M_RSHIFT)]; // (one doc-id per entry: the weight byte was the answer)
                    }
                    return true;
                };
                static_list_loop<1, RL>(nt, load_hint);
                auto test_hint = [&](auto ic) __attribute__((always_inline)) {
                    constexpr uint32_t i = decltype(ic)::value;
                    ok = ok && ((h[i] == 255u) | (h[i] == rmh_code(c, cx.m(i, M_RSHIFT))));
                    return true;
                };
                static_list_loop<1, RL>(nt, test_hint);
            }
            return ok;
        };
        cx.s_bytes += 4;
        ++cx.s_bm_examined;
        uint32_t lo = 0, floor_tick = 1;
        uint64_t okm0 = ~0ull, okm1 = ~0ull; // and / and_freq: candidates of list 0's block the range tables have not ruled out
        uint32_t part_blk = 0xFFFFFFFFu; // block of list 0 whose norm_lens / list-0 scores are in L.nl
        // ---- list 0 as a STREAM (block indexes with the interleaved skip table). The driving list is walked front to
        // back, most of its blocks only to find that none of their documents can be a result, so what a step costs is its
        // dependent memory round trips. The stream keeps a 64-entry window of the list's table rows in registers (lane j:
        // {block_max, end offset} and the block weight of entry s_first + j; lane 0 is the row BEFORE the first block the
        // window can serve, whose block_max / end offset give that block's base / start): "which block is next" is a ballot
        // over registers, a block's table words cost no load, and the bytes of the block that will be taken after the
        // current one are requested while the current one is still being worked on (pf_d0 / pf_d1: 512 B, two dwords per lane).
        // The freq_index layouts stream the same way over their chunk directory: the window holds cmax[] (a chunk's last
        // doc-id) and the chunk weights, and what is requested ahead is the next chunk's 12-dword directory entry (its bit
        // positions: the first of the two dependent loads a chunk decode starts with).
        const bool pstream = cx.is_pef();
        const bool stream0 = pstream || cx.skip;
        const uint2* const tab0 = (stream0 && !pstream) ? cx.skip + cx.m(0, M_PBASE) : nullptr;
        const uint32_t* const cmax0 = pstream ? (const uint32_t*)cx.ptr(0, M_MAXS_LO) : nullptr;
        const uint32_t* const ent0 = pstream ? (const uint32_t*)cx.ptr(0, M_END_LO) : nullptr;
        const uint8_t* data0 = nullptr;
        uint32_t s_first = 0, pf_blk = 0xFFFFFFFFu, pf_d0 = 0, pf_d1 = 0, pf_x = 0;
        uint2 s_e = make_uint2(0xFFFFFFFFu, 0u);
        float s_w = 0.f, s_rb = 0.f;
        bool s_none = false; // some other list has no posting at all inside the block's doc-id span: nothing to intersect
        auto s_fill = [&](uint32_t first) __attribute__((always_inline)) {
            s_first = first;
            const uint32_t idx = first + lane;
            s_e = make_uint2(0xFFFFFFFFu, 0u);
            s_w = 0.f;
            if (idx < u.blk_end) {
                if (pstream) s_e.x = cmax0[idx]; else s_e = tab0[idx];
                if (RANKED && w0tab) s_w = w0tab[idx];
            }
            s_none = false;
            {
                s_rb = RANKED ? __uint_as_float(cx.m(0, M_SUF)) : 0.f; // what the other lists can add to a document of the block: their list maxima, or
                if (use_rmw) {
                    // ... with range tables the largest entry each of them has over the block's own doc-id span [base, block_max],
                    // read from the level of the table whose entries are wide enough for <= 16 of them to cover the span
                    // (a lane serves the block of its table row; 16 independent byte loads per list, once per 63 blocks)
                    const uint32_t prev_max = (uint32_t)__shfl_up((int)s_e.x, 1);
                    const uint32_t base = (lane == 0) ? 0u : prev_max + 1u, top = s_e.x;
                    const bool row = idx < u.blk_end && (lane > 0 || idx == 0) && top != 0xFFFFFFFFu && base <= top;
                    float acc = 0.f;
                    auto one_list = [&](auto jc) __attribute__((always_inline)) {
                        constexpr uint32_t j = decltype(jc)::value;
                        if (j >= nt) return;
                        const uint32_t sh = cx.m(j, M_RSHIFT);
                        const RmwLevels g(a.num_docs, sh);
                        const uint8_t* tb = rmw + 64ull * cx.m(j, M_RBASE);
                        uint32_t best = 255u; // (the list maximum)
                        {   // branch-free: a lane without a row reads entry 0 and discards it
                            const uint32_t b2 = row ? base : 0u, t2 = row ? top : 0u;
                            uint32_t lsh = sh, lvl = 0;
                            while (lvl < 2 && (t2 >> lsh) - (b2 >> lsh) >= 16u) { lsh += 6; ++lvl; }
                            const uint32_t lo = b2 >> lsh, hi = t2 >> lsh;
                            const bool fits = hi - lo < 16u;
                            const uint32_t m = max_of_bytes16(tb + g.off[lvl] + (fits ? lo : 0u), fits ? hi - lo + 1u : 1u);
                            if (row && fits) best = m;
                        }
                        s_none = s_none || best == 0u;
                        if constexpr (RANKED) acc = acc + __uint_as_float(cx.m(j, M_RSCALE)) * (float)best;
                    };
                    static_loop_down<RL, 1>(one_list);
                    s_rb = acc;
                }
            }
        };
        // blocks >= from of the window that are worth a visit: inside the unit and (ranked, once bounds can prune) able to
        // hold a document that enters the heap going by the block's weight + the other lists' list maxima
        auto s_live = [&](uint32_t from) __attribute__((always_inline)) -> uint64_t {
            const uint32_t idx = s_first + lane;
            bool ok = idx >= from && idx < u.blk_end && (lane > 0 || idx == 0) && !s_none;
            if constexpr (RANKED) {
                if (bmw && can_prune()) {
                    const float qw0 = __uint_as_float(cx.m(0, M_QW));
                    ok = ok && tk.would_enter((qw0 * s_w + s_rb) * BOUND_SLACK);
                }
            }
            return ballot(ok);
        };
        auto s_next = [&](uint32_t from) __attribute__((always_inline)) -> uint32_t { // first block >= from worth a visit, or blk_end
            for (;;) {
                if (from >= u.blk_end) return u.blk_end;
                const uint64_t hit = s_live(from);
                if (hit) return s_first + (uint32_t)__builtin_ctzll(hit);
                if (s_first + 64 >= u.blk_end) return u.blk_end;
                s_fill(s_first + 63);
                from = from > s_first + 1 ? from : s_first + 1;
            }
        };
        if (stream0) {
            if (!pstream) {
                const uint8_t* maxs0 = cx.ptr(0, M_MAXS_LO);
                const uint32_t nb0 = cx.m(0, M_NB);
                data0 = maxs0 + 4ull * nb0 + 4ull * (nb0 - 1);
            }
            s_fill(u.blk_begin ? u.blk_begin - 1 : 0);
        }
        // list 0 moves on: `want` = first block with block_max >= lo (or the unit's first block)
        uint32_t want = u.blk_begin;
        bool have_bi = false;
        typename decltype(cx)::BlockInfo bi0;
        bool finished = false;
        bool need0 = true;
#ifdef DS2I_PHASE_TIMING
        cx.s_phase[PH_UNIT] += __builtin_readcyclecounter() - unit_t0;
#endif
        while (!finished) {
            ++cx.s_rounds;
#ifdef DS2I_PHASE_TIMING
            const unsigned long long round_t0 = __builtin_readcyclecounter(); // PH_PROLOG = rounds that end at the range-table test
#endif
            if (stream0 && (need0 || lo > cx.m(0, M_BMAX))) { // list 0 supplies the candidates of this round
                // (lo never exceeds block_max + 1 of list 0's block -- the window is cut at it -- so the next block with
                // block_max >= lo is simply the next one)
                const uint32_t from = need0 ? u.blk_begin : cx.m(0, M_CUR) + 1;
                if (from >= u.blk_end) break;
                cx.s_bm_examined += 1;
                cx.s_bytes += 4;
                // (the shared histogram costs an L2 round trip: consulted every DS2I_FLOOR_EVERY-th block of list 0; every
                // block: -3 %, every 16th: -6 % -- the staler floor costs decodes)
                if (shared_floor && (floor_tick++ & (DS2I_FLOOR_EVERY - 1)) == 0) { PT_BEGIN(cx); adopt_floor(); PT_END(cx, PH_FLOOR); }
                PT_BEGIN(cx);
                const uint32_t blk2 = s_next(from);
                if (blk2 >= u.blk_end) break;
                const uint32_t f = blk2 - s_first, fp = f ? f - 1 : 0;
                bi0.bmax = bcast(s_e.x, f);
                bi0.next_ep = bcast(s_e.y, f);
                bi0.base = blk2 ? bcast(s_e.x, fp) + 1u : 0u;
                bi0.ep = blk2 ? bcast(s_e.y, fp) : 0u;
                const bool staged = pf_blk == blk2;
                if (staged && !pstream) { // the block's bytes were requested a block ago: from registers into the staging window
                    const uint8_t* p = data0 + bi0.ep;
                    cx.win.gbase = (const uint8_t*)((uintptr_t)p & ~(uintptr_t)3);
                    cx.win.nbytes = 512;
                    cx.win.st[lane] = pf_d0;
                    cx.win.st[lane + 64] = pf_d1;
                    if (cx.side()) { cx.exc[lane] = pf_x; cx.slot_blk = cx.m(0, M_PBASE) + blk2; } // (its side slot came with them)
                    wave_sync();
                }
                PT_END(cx, PH_STREAM);
                if (pstream) cx.decode_docs_pef(0, blk2, staged ? &pf_d0 : nullptr);
                else cx.decode_docs(0, blk2, &bi0, staged);
#ifdef DS2I_PHASE_TIMING
                cx.s_phase[PH_C_VISIT] += 1;
#endif
                need0 = false;
                { // request the bytes of the block that is next as things stand (the heap may still rule it out later)
                    PT_BEGIN(cx);
                    const uint64_t nx = s_live(blk2 + 1);
                    pf_blk = 0xFFFFFFFFu;
                    if (nx) {
                        const uint32_t fn = (uint32_t)__builtin_ctzll(nx);
                        if (pstream) { // the chunk's directory entry (lanes 0..11) and its cmax (lane 12), as decode_docs_pef reads them
                            const uint32_t nb2 = s_first + fn, cm = bcast(s_e.x, fn);
                            pf_d0 = lane == PC_WORDS ? cm : 0u;
                            if (lane < PC_WORDS) pf_d0 = ent0[(size_t)nb2 * PC_WORDS + lane];
                        } else {
                            const uint32_t* g = (const uint32_t*)((uintptr_t)(data0 + bcast(s_e.y, fn - 1)) & ~(uintptr_t)3);
                            pf_d0 = g[lane];
                            pf_d1 = g[lane + 64];
                            if (cx.side()) pf_x = cx.xslots[(size_t)XSLOT_DW * (cx.m(0, M_PBASE) + s_first + fn) + lane];
                        }
                        pf_blk = s_first + fn;
                    }
                    PT_END(cx, PH_PREFETCH);
                }
                if constexpr (!RANKED) {
                    if (use_rmw) { // once per block of list 0: who can be a member of every other list at all
                        const uint32_t n0c = L.docs[0][lane], n1c = L.docs[0][lane + 64];
                        okm0 = ballot(and_filter(n0c, n0c != 0xFFFFFFFFu));
                        okm1 = ballot(and_filter(n1c, n1c != 0xFFFFFFFFu));
                    }
                }
            } else if (need0 || lo > cx.m(0, M_BMAX)) { // (freq_index layouts, or no skip table: the search-based form)
                const bool tabbed = META::SKIPTAB && !cx.is_pef() && cx.skip;
                if (!need0) {
                    const uint32_t cur = cx.m(0, M_CUR);
                    { PT_BEGIN(cx); want = tabbed ? cx.find_block_info(0, cur + 1, lo, bi0) : cx.find_block(0, cur + 1, lo); PT_END(cx, PH_FIND); }
                    have_bi = tabbed;
                    cx.s_bm_examined += want - cur;
                    cx.s_bytes += 4ull * (want - cur);
                }
                if (want >= u.blk_end) break;
                // (the shared histogram costs an L2 round trip: consulted every DS2I_FLOOR_EVERY-th block of list 0)
                if (shared_floor && (floor_tick++ & (DS2I_FLOOR_EVERY - 1)) == 0) adopt_floor();
                const uint32_t blk2 = skip_list0(want);
                if (blk2 >= u.blk_end) break;
                cx.decode_docs(0, blk2, (have_bi && blk2 == want) ? &bi0 : nullptr);
                need0 = false;
                if constexpr (!RANKED) {
                    if (use_rmw) { // once per block of list 0: who can be a member of every other list at all
                        const uint32_t n0c = L.docs[0][lane], n1c = L.docs[0][lane + 64];
                        okm0 = ballot(and_filter(n0c, n0c != 0xFFFFFFFFu));
                        okm1 = ballot(and_filter(n1c, n1c != 0xFFFFFFFFu));
                    }
                }
            }
            uint32_t hi = cx.m(0, M_BMAX);
            const uint32_t c0 = L.docs[0][lane], c1 = L.docs[0][lane + 64];
            bool al0 = c0 >= lo && c0 != 0xFFFFFFFFu, al1 = c1 >= lo && c1 != 0xFFFFFFFFu;
            if constexpr (!RANKED) {
                al0 = al0 && ((okm0 >> lane) & 1);
                al1 = al1 && ((okm1 >> lane) & 1);
            }
            // ranked_and scores PROGRESSIVELY: pa0 / pa1 are the running float32 sums of this lane's two candidates in
            // list order (queries.hpp:372-380). `sf` (wave-uniform) = the heap is full or a floor is known, so bounds
            // can prune: then the list-0 term scores of the whole block are computed up front (once per block, kept in
            // LDS); otherwise they are computed for the candidates that survive list 1, when they are first needed.
            const bool sf = RANKED && bmw && (use_rmw || can_prune());
            float pa0 = 0.f, pa1 = 0.f;
            uint32_t ql0 = 0, qh0 = 0, ql1 = 0, qh1 = 0; // this lane's two candidates: packed range-table bytes
            bool have_p = false;
            if constexpr (RANKED) {
                if (sf || nt == 1) {
                    const uint32_t cur0 = cx.m(0, M_CUR);
                    if (part_blk != cur0) { // once per block of list 0: its freqs, the norm_lens and the list-0 term scores
                        const float qw0 = __uint_as_float(cx.m(0, M_QW));
                        bool v0 = c0 != 0xFFFFFFFFu, v1 = c1 != 0xFFFFFFFFu;
                        float r0 = __uint_as_float(cx.m(0, M_SUF)), r1 = r0;
                        if (sf && use_rmw) {
                            // Range tables first, with the BLOCK's weight standing in for the candidates' list-0 scores: most
                            // blocks of the driving list hold no document that is both inside every other list's ranges and
                            // able to enter the heap -- those are left without decoding their freqs or touching a norm_len.
                            PT_BEGIN(cx);
                            const float wblk = qw0 * (stream0 ? __uint_as_float(bcast(__float_as_uint(s_w), cur0 - s_first))
                                                              : w0tab[cur0]); // (uniform load, in flight with the gathers)
                            v0 = rmw_gather(c0, v0, ql0, qh0);
                            v1 = rmw_gather(c1, v1, ql1, qh1);
                            r0 = rmw_rest(ql0, qh0, 0);
                            r1 = rmw_rest(ql1, qh1, 0);
                            v0 = v0 && tk.would_enter((wblk + r0) * BOUND_SLACK);
                            v1 = v1 && tk.would_enter((wblk + r1) * BOUND_SLACK);
                            if (a.rmh && (ballot(v0) | ballot(v1))) {
                                // membership hints (BatchArgs::rmh): for the candidates the weight bytes let through, every other
                                // list says WHICH document of the candidate's range is its own (where it is the only one there):
                                // a candidate elsewhere in that range is in no intersection with the list -- settled by one more
                                // byte per list instead of a block search and a block decode. All loads first, then the tests.
                                const long long hd = (long long)(a.rmh - a.rmw);
                                uint32_t h0[RL] = {}, h1[RL] = {};
                                auto load_hint = [&](auto ic) __attribute__((always_inline)) {
                                    constexpr uint32_t i = decltype(ic)::value;
                                    const uint8_t* ht = rmw + 64ull * cx.m(i, M_RBASE) + hd;
                                    const uint32_t sh = cx.m(i, M_RSHIFT);
                                    h0[i] = (v0 && sh != 0u) ? (uint32_t)ht[c0 >> sh] : 255u; // (one doc-id per entry: the weight byte was the answer)
                                    h1[i] = (v1 && sh != 0u) ? (uint32_t)ht[c1 >> sh] : 255u;
                                    return true;
                                };
                                static_list_loop<1, RL>(nt, load_hint);
                                auto test_hint = [&](auto ic) __attribute__((always_inline)) {
                                    constexpr uint32_t i = decltype(ic)::value;
                                    const uint32_t sh = cx.m(i, M_RSHIFT);
                                    v0 = v0 && ((h0[i] == 255u) | (h0[i] == rmh_code(c0, sh)));
                                    v1 = v1 && ((h1[i] == 255u) | (h1[i] == rmh_code(c1, sh)));
                                    return true;
                                };
                                static_list_loop<1, RL>(nt, test_hint);
                            }
                            PT_END(cx, PH_PROBE);
#ifdef DS2I_PHASE_TIMING
                            cx.s_phase[PH_C_SURV1] += __builtin_popcountll(ballot(v0)) + __builtin_popcountll(ballot(v1));
#endif
                            if (!(ballot(v0) | ballot(v1))) {
#ifdef DS2I_PHASE_TIMING
                                cx.s_phase[PH_PROLOG] += __builtin_readcyclecounter() - round_t0;
                                cx.s_phase[PH_INSERT] += 1; // (count of such rounds)
#endif
                                if (hi == 0xFFFFFFFFu) break;
                                lo = hi + 1;
                                continue;
                            }
                            L.qb[lane] = ql0;
                            L.qb[lane + 64] = ql1;
                            if constexpr (TMAX > 4) { L.qb2[lane] = qh0; L.qb2[lane + 64] = qh1; }
                        }
                        if (!cx.freqs_ready(0)) cx.decode_freqs(0);
                        PT_BEGIN(cx);
                        const uint32_t f0 = L.freqs[0][lane], f1 = L.freqs[0][lane + 64];
                        if (sf) {
                            // The 4-byte norm_len gather is the path's largest source of memory traffic (a 64-byte
                            // request each). doc_term_weight falls with norm_len, so the freq alone bounds the term
                            // score: a posting whose bound (shortest document of the collection) cannot reach the heap
                            // is dropped before its norm_len is fetched. The heap only tightens, so the verdict holds
                            // for every later round of this block (-inf marks the dropped postings).
                            // With range tables the other lists' part of the bound is per candidate (r0 / r1 above).
                            v0 = v0 && tk.would_enter((qw0 * doc_term_weight(f0, a.min_norm_len) + r0) * BOUND_SLACK);
                            v1 = v1 && tk.would_enter((qw0 * doc_term_weight(f1, a.min_norm_len) + r1) * BOUND_SLACK);
                        }
                        const float n0 = v0 ? a.norm_lens[c0] : -1.f, n1 = v1 ? a.norm_lens[c1] : -1.f;
                        L.nl[lane] = n0;
                        L.nl[lane + 64] = n1;
                        L.part0[lane] = v0 ? qw0 * doc_term_weight(f0, n0) : -__builtin_inff();
                        L.part0[lane + 64] = v1 ? qw0 * doc_term_weight(f1, n1) : -__builtin_inff();
                        part_blk = cur0;
#ifdef DS2I_PHASE_TIMING
                        {
                            const float p0_ = L.part0[lane], p1_ = L.part0[lane + 64];
                            cx.s_phase[PH_C_SURV2] += __builtin_popcountll(ballot(v0 && tk.would_enter((p0_ + r0) * BOUND_SLACK))) +
                                                      __builtin_popcountll(ballot(v1 && tk.would_enter((p1_ + r1) * BOUND_SLACK)));
                        }
#endif
                        const uint32_t nv = (uint32_t)(__builtin_popcountll(ballot(v0)) + __builtin_popcountll(ballot(v1)));
                        cx.s_bytes += 4ull * nv;
                        cx.s_scored += nv;
                        wave_sync();
                        PT_END(cx, PH_SCORE);
                    }
                    pa0 = L.part0[lane]; // list-0 term scores of this lane's two candidates (-inf: dropped at block init)
                    pa1 = L.part0[lane + 64];
                    have_p = true;
                    if (sf) {
                        float r0 = __uint_as_float(cx.m(0, M_SUF)), r1 = r0;
                        if (use_rmw) {
                            ql0 = L.qb[lane];
                            ql1 = L.qb[lane + 64];
                            if constexpr (TMAX > 4) { qh0 = L.qb2[lane]; qh1 = L.qb2[lane + 64]; }
                            r0 = rmw_rest(ql0, qh0, 0);
                            r1 = rmw_rest(ql1, qh1, 0);
                        }
                        // (pa >= 0 excludes the dropped postings explicitly: while the heap is not full would_enter(-inf) holds)
                        al0 = al0 && pa0 >= 0.f && tk.would_enter((pa0 + r0) * BOUND_SLACK);
                        al1 = al1 && pa1 >= 0.f && tk.would_enter((pa1 + r1) * BOUND_SLACK);
                    }
                }
            }
#ifdef DS2I_PHASE_TIMING
            cx.s_phase[PH_C_LIVEROUNDS] += 1;
#endif
            bool pruned = false;
            auto probe_list = [&](auto ic) __attribute__((always_inline)) -> bool {
                const uint32_t i = ic;
                if constexpr (!RANKED && !WITH_FREQS) { if ((bm_lists >> i) & 1u) return true; } // settled by its bitmap
                uint64_t b0 = ballot(al0), b1 = ballot(al1);
                if (!(b0 | b1)) return false;
                uint32_t amin = b0 ? bcast(c0, (uint32_t)__builtin_ctzll(b0)) : bcast(c1, (uint32_t)__builtin_ctzll(b1));
                if (cx.m(i, M_CUR) == 0xFFFFFFFFu || amin > cx.m(i, M_BMAX)) {
                    uint32_t cur = cx.m(i, M_CUR);
                    uint32_t blk, nbmax = 0;
                    float wnew = 0.f;
                    typename decltype(cx)::BlockInfo bi;
                    const bool tabbed = META::SKIPTAB && !cx.is_pef() && cx.skip;
                    const float* wtab = (RANKED && sf) ? bmw + cx.m(i, M_PBASE) : nullptr;
                    {
                        PT_BEGIN(cx);
                        if (tabbed) { blk = cx.find_block_info(i, cur + 1, amin, bi, wtab, wnew); nbmax = bi.bmax; }
                        else blk = cx.find_block(i, cur + 1, amin, nbmax, wtab, wnew);
                        PT_END(cx, PH_FIND);
                    }
                    if (blk >= cx.m(i, M_NB)) { // list i has nothing >= amin: no further match exists
                        cx.s_bm_examined += 1;
                        cx.s_bytes += 4;
                        al0 = al1 = false;
                        finished = true;
                        return false;
                    }
                    // a lazily bound list is positioned by one 64-ary search, not a scan from block 0
                    cx.s_bm_examined += (cur == 0xFFFFFFFFu) ? 1u : blk - cur;
                    cx.s_bytes += 4ull * ((cur == 0xFFFFFFFFu) ? 1u : blk - cur);
                    bool skip_decode = false;
                    if constexpr (RANKED) {
                        if (sf) {
                            // best alive partial score inside [lo, min(hi, block_max)] + this block's max weight + the
                            // later lists' maxima: if that cannot enter the heap the block is not even decoded
                            const uint32_t wh = nbmax < hi ? nbmax : hi;
                            const float cbw = __uint_as_float(cx.m(i, M_QW)) * wnew;
                            float pm, p1, tail = __uint_as_float(cx.m(i, M_SUF));
                            if (use_rmw) { // per candidate: its partial + min(block weight, its own byte bound in list i) + its later lists
                                float t0 = cbw, t1 = cbw;
                                if constexpr (std::is_same<decltype(ic), uint32_t>::value) {
                                    // (run-time list slot: the 5-8-list class; keep the block weight for list i)
                                } else {
                                    const float b0 = rmw_term(ql0, qh0, ic), b1 = rmw_term(ql1, qh1, ic);
                                    t0 = b0 < cbw ? b0 : cbw;
                                    t1 = b1 < cbw ? b1 : cbw;
                                }
                                pm = (al0 && c0 <= wh) ? (pa0 + t0) + rmw_rest(ql0, qh0, i) : 0.f;
                                p1 = (al1 && c1 <= wh) ? (pa1 + t1) + rmw_rest(ql1, qh1, i) : 0.f;
                                tail = 0.f;
                            } else {
                                pm = (al0 && c0 <= wh) ? pa0 + cbw : cbw;
                                p1 = (al1 && c1 <= wh) ? pa1 + cbw : cbw;
                            }
                            pm = p1 > pm ? p1 : pm; // scores are >= 0: their bit patterns order like the values
                            pm = __uint_as_float(bcast(wave_incl_max_scan(__float_as_uint(pm)), 63));
                            if (!tk.would_enter((pm + tail) * BOUND_SLACK)) {
                                hi = wh;
                                skip_decode = true;
                            }
                        }
                    }
                    if (skip_decode) {
                        pruned = true;
                        return false;
                    }
                    cx.decode_docs(i, blk, tabbed ? &bi : nullptr);
#ifdef DS2I_PHASE_TIMING
                    cx.s_phase[PH_C_BDOCS] += 1;
#endif
                }
                PT_BEGIN(cx);
                uint32_t bm = cx.m(i, M_BMAX);
                hi = bm < hi ? bm : hi;
                bool w0 = al0 && c0 <= hi, w1 = al1 && c1 <= hi;
                const uint32_t* d = L.docs[i];
                uint64_t wb0 = ballot(w0), wb1 = ballot(w1);
                uint32_t nw = (uint32_t)(__builtin_popcountll(wb0) + __builtin_popcountll(wb1));
                uint32_t p0 = 0, p1 = 0;
                if (nw > 24) {
                    al0 = member_bsearch(d, c0, w0, p0);
                    al1 = member_bsearch(d, c1, w1, p1);
                } else {
                    // few candidates: broadcast each, two equality ballots over the block
                    const uint32_t d0 = d[lane], d1 = d[lane + 64];
                    uint64_t r0 = 0, r1 = 0;
                    for (int half = 0; half < 2; ++half) {
                        uint64_t todo = half ? wb1 : wb0;
                        while (todo) {
                            uint32_t src = (uint32_t)__builtin_ctzll(todo);
                            todo &= todo - 1;
                            uint32_t c = bcast(half ? c1 : c0, src);
                            uint64_t e0 = ballot(d0 == c), e1 = ballot(d1 == c);
                            if (e0 | e1) {
                                uint32_t pp = e0 ? (uint32_t)__builtin_ctzll(e0) : 64u + (uint32_t)__builtin_ctzll(e1);
                                if (half) { r1 |= 1ull << src; if (lane == src) p1 = pp; }
                                else { r0 |= 1ull << src; if (lane == src) p0 = pp; }
                            }
                        }
                    }
                    al0 = (r0 >> lane) & 1;
                    al1 = (r1 >> lane) & 1;
                }
                PT_END(cx, PH_MEMBER);
                if constexpr (RANKED) { // members take list i's term score at once
                    if (ballot(al0) | ballot(al1)) {
                        if (!have_p) { // (only possible at list 1) list-0 term scores of the surviving candidates
                            if (!cx.freqs_ready(0)) cx.decode_freqs(0);
                            const float qw0 = __uint_as_float(cx.m(0, M_QW));
                            const float n0 = al0 ? a.norm_lens[c0] : 0.f, n1 = al1 ? a.norm_lens[c1] : 0.f;
                            L.nl[lane] = n0;
                            L.nl[lane + 64] = n1;
                            pa0 = al0 ? qw0 * doc_term_weight(L.freqs[0][lane], n0) : 0.f;
                            pa1 = al1 ? qw0 * doc_term_weight(L.freqs[0][lane + 64], n1) : 0.f;
                            part_blk = 0xFFFFFFFFu; // L.nl now holds this round's survivors only
                            have_p = true;
                            const uint32_t nv = (uint32_t)(__builtin_popcountll(ballot(al0)) + __builtin_popcountll(ballot(al1)));
                            cx.s_bytes += 4ull * nv;
                            cx.s_scored += nv;
                        }
#ifdef DS2I_PHASE_TIMING
                        if (!cx.freqs_ready(i)) cx.s_phase[PH_C_BFREQS] += 1;
#endif
                        if (!cx.freqs_ready(i)) cx.decode_freqs(i);
                        const float qw = __uint_as_float(cx.m(i, M_QW));
                        const uint32_t* f = cx.F(i);
                        if (al0) pa0 = pa0 + qw * doc_term_weight(f[p0], L.nl[lane]);
                        if (al1) pa1 = pa1 + qw * doc_term_weight(f[p1], L.nl[lane + 64]);
                        if (sf) { // who cannot reach the heap any more drops out before the next list is touched
                            float r0 = __uint_as_float(cx.m(i, M_SUF)), r1 = r0;
                            if (use_rmw) { r0 = rmw_rest(ql0, qh0, i); r1 = rmw_rest(ql1, qh1, i); }
                            al0 = al0 && tk.would_enter((pa0 + r0) * BOUND_SLACK);
                            al1 = al1 && tk.would_enter((pa1 + r1) * BOUND_SLACK);
                        }
                    }
                    return true;
                }
                if constexpr (WITH_FREQS && !RANKED) {
                    if (al0) L.pos[i][lane] = (uint8_t)p0;
                    if (al1) L.pos[i][lane + 64] = (uint8_t)p1;
                }
                return true;
            };
            DS2I_LIST_LOOP(1, probe_list)
            if (RANKED && pruned) { // the window [lo, hi] holds no document that could enter the heap
                if (hi == 0xFFFFFFFFu) break;
                lo = hi + 1;
                continue;
            }
            // candidates that survived every list and lie inside the window are matches
            al0 = al0 && c0 <= hi;
            al1 = al1 && c1 <= hi;
            const uint64_t s0 = ballot(al0), s1 = ballot(al1);
            const uint32_t ns = (uint32_t)(__builtin_popcountll(s0) + __builtin_popcountll(s1));
            if (ns) {
                if (a.out_matches) {
                    const uint64_t lt = (1ull << lane) - 1;
                    unsigned long long i0 = count + __builtin_popcountll(s0 & lt);
                    unsigned long long i1 = count + __builtin_popcountll(s0) + __builtin_popcountll(s1 & lt);
                    if (al0 && i0 < mcap) a.out_matches[mbase + i0] = c0;
                    if (al1 && i1 < mcap) a.out_matches[mbase + i1] = c1;
                }
                count += ns;
                if constexpr (WITH_FREQS && !RANKED) { // and_query<with_freqs> touches every matching posting's freq
                    wave_sync(); // L.pos writes visible
                    unsigned long long fs = 0; // freqs are u32: the checksum must not wrap at 2^32
                    auto freq_list = [&](auto ic) __attribute__((always_inline)) -> bool {
                        const uint32_t i = ic;
                        if (!cx.m(i, M_FDEC)) cx.decode_freqs(i);
                        const uint32_t* f = L.freqs[i];
                        uint32_t f0 = 0, f1 = 0;
                        if (al0) f0 = f[i ? L.pos[i][lane] : lane];
                        if (al1) f1 = f[i ? L.pos[i][lane + 64] : lane + 64];
                        fs += (unsigned long long)f0 + f1;
                        return true;
                    };
                    DS2I_LIST_LOOP(0, freq_list)
                    fsum += fs; // (this lane's share: reduced over the wave once, when the unit ends)
                }
                if constexpr (RANKED) {
                    // pa0 / pa1 are complete scores now; only those that can enter the heap are inserted (serial, rare once warm)
#ifdef DS2I_PHASE_TIMING
                    const unsigned long long tk_t0 = __builtin_readcyclecounter();
#endif
                    for (int half = 0; half < 2; ++half) {
                        const bool al = half ? al1 : al0;
                        const float sc = half ? pa1 : pa0;
                        uint64_t todo = ballot(al && tk.would_enter(sc));
                        while (todo) {
                            uint32_t src = (uint32_t)__builtin_ctzll(todo);
                            todo &= todo - 1;
                            const float v = __uint_as_float(bcast(__float_as_uint(sc), src));
#ifdef DS2I_PHASE_TIMING
                            cx.s_phase[PH_C_HEAP] += 1;
#endif
                            if (TK_INSERT(tk, v, bcast(half ? c1 : c0, src)) && shared_floor && lane == 0) sh.add(v);
                        }
                    }
#ifdef DS2I_PHASE_TIMING
                    cx.s_phase[PH_TOPK] += __builtin_readcyclecounter() - tk_t0;
#endif
                }
            }
            if (hi == 0xFFFFFFFFu) break;
            lo = hi + 1;
        }
#ifdef DS2I_PHASE_TIMING
        cx.s_phase[PH_TOTAL] += __builtin_readcyclecounter() - unit_t0;
#endif
        if constexpr (WITH_FREQS && !RANKED) {
            for (int o = 32; o; o >>= 1) fsum += __shfl_xor(fsum, o);
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
        if (STATS && a.unit_clock && lane == 0) { a.unit_clock[2ull * uid] = t_unit; a.unit_clock[2ull * uid + 1] = wall_clock64(); }
    }
    cx.flush_stats(a.stats);
}

// Merges the partial results of split queries: counts add up, the top-k of a union is the top-k of
// the parts' top-ks (scores are per-document, so the merged multiset equals the sequential one).
__global__ void __launch_bounds__(64) DS2I_KN(k_merge)(MergeArgs a) {
    const uint32_t lane = lane_id();
    for (uint32_t w = blockIdx.x; w < a.nsplit; w += gridDim.x) {
        const uint32_t q = a.split_queries[w];
        const uint32_t u0 = a.q_unit_off[q], u1 = a.q_unit_off[q + 1];
        unsigned long long count = 0, fsum = 0;
        for (uint32_t u = u0 + lane; u < u1; u += 64) { count += a.unit_count[u]; fsum += a.unit_freq_sum[u]; }
        for (int o = 32; o; o >>= 1) {
            count += __shfl_xor(count, o);
            fsum += __shfl_xor(fsum, o);
        }
        RTopK tk;
        tk.init(a.k);
        if (a.ranked) {
            for (uint32_t u = u0; u < u1; ++u) {
                const uint32_t len = a.unit_topk_len[u];
                float v = lane < len ? a.unit_topk[(size_t)u * a.k + lane] : -__builtin_inff();
#ifdef DS2I_DOCS_TU
                const uint32_t vd = lane < len ? a.unit_topk_docs[(size_t)u * a.k + lane] : 0xFFFFFFFFu;
#endif
                uint64_t todo = ballot(lane < len && tk.would_enter(v));
                while (todo) {
                    uint32_t src = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    TK_INSERT(tk, __uint_as_float(bcast(__float_as_uint(v), src)), bcast(vd, src));
                }
            }
            store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
        }
        if (lane == 0) {
            a.out_count[q] = a.ranked ? tk.n : count;
            if (a.out_freq_sum) a.out_freq_sum[q] = fsum;
        }
    }
}

// ... and of ranked_and batches with 64 < k <= 64 NK (the stream kernels' big heaps, ranked_stream.hip)
template <int NK>
__global__ void __launch_bounds__(64) DS2I_KN(k_merge_big)(MergeArgs a) {
    const uint32_t lane = lane_id();
    for (uint32_t w = blockIdx.x; w < a.nsplit; w += gridDim.x) {
        const uint32_t q = a.split_queries[w];
        const uint32_t u0 = a.q_unit_off[q], u1 = a.q_unit_off[q + 1];
        unsigned long long count = 0, fsum = 0;
        for (uint32_t u = u0 + lane; u < u1; u += 64) { count += a.unit_count[u]; fsum += a.unit_freq_sum[u]; }
        for (int o = 32; o; o >>= 1) {
            count += __shfl_xor(count, o);
            fsum += __shfl_xor(fsum, o);
        }
        RTopKBig<NK> tk;
        tk.init(a.k);
        if (a.ranked) {
            for (uint32_t u = u0; u < u1; ++u) {
                const uint32_t len = a.unit_topk_len[u];
                for (uint32_t r0 = 0; r0 < len; r0 += 64) { // (a unit's scores are in descending order: once a row enters nothing, the rest cannot)
                    const uint32_t i = r0 + lane;
                    float v = i < len ? a.unit_topk[(size_t)u * a.k + i] : -__builtin_inff();
#ifdef DS2I_DOCS_TU
                    const uint32_t vd = i < len ? a.unit_topk_docs[(size_t)u * a.k + i] : 0xFFFFFFFFu;
#endif
                    uint64_t todo = ballot(i < len && tk.would_enter(v));
                    if (!todo) break;
                    while (todo) {
                        uint32_t src = (uint32_t)__builtin_ctzll(todo);
                        todo &= todo - 1;
                        TK_INSERT(tk, __uint_as_float(bcast(__float_as_uint(v), src)), bcast(vd, src));
                    }
                }
            }
            store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
        }
        if (lane == 0) {
            a.out_count[q] = a.ranked ? tk.n : count;
            if (a.out_freq_sum) a.out_freq_sum[q] = fsum;
        }
    }
}
