// wand / maxscore / ranked_or without side slots or range tables (k_disjunctive, k_union_topk) and or / or_freq as a stream (k_union)
// (part of kernels.hip -- included inside its anonymous namespace, once per translation unit of the list-count classes; not a
// stand-alone header)
// ------------------------------------------------------------------ block-synchronous disjunctive top-k
// wand / maxscore / ranked_or all return the top-k of the UNION of the query's lists (queries.hpp:200-319, 404-476,
// 478-591; the reference's own ranked test holds them equal, test_ranked_queries.cpp:39-57). The document-at-a-time
// traversals of the reference (k_daat above) advance one document per step; here a step is a WINDOW of doc-ids:
//   * lists are ordered by max score, upper_bounds[] are the prefix sums and the first `non_ess` lists are
//     non-essential exactly as in maxscore_query (queries.hpp:529-547): a document that occurs in them only cannot
//     enter the heap. The threshold starts at the ranked_and seed (every AND result is an OR result).
//   * every essential list keeps one decoded block; the window is [lo, min of their block_max], so all postings of
//     the essential lists inside the window sit in LDS. Each posting is a candidate, owned by the first essential list
//     that contains it (later lists mark their copy as a duplicate);
//   * a candidate's max-score bound (lists it was found in + all non-essential lists) is tested first, the survivors
//     are scored exactly: essential lists by position, non-essential lists probed from the highest bound down while
//     score + upper_bound can still enter (queries.hpp:553-564), 128 candidates at a time.
// Position (0..127) of one candidate in each of the query's lists, 7 bits per list slot, in registers: the union kernels
// are capped by LDS per wave (residency hides their dependent round trips), so what a lane knows about its own two
// candidates stays out of LDS. <=4 lists fit one dword, <=8 one qword, 16 two.
template <int TMAX>
struct PosPack {
    typedef typename std::conditional<(TMAX <= 4), uint32_t, unsigned long long>::type word_t;
    static constexpr int PER = TMAX <= 4 ? 4 : 9, NW = (TMAX + PER - 1) / PER;
    word_t w[NW];
    DS2I_DEV void clear() {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 0;
    }
    DS2I_DEV void set(uint32_t x, uint32_t pos) { // x wave-uniform
        if (NW == 1 || x < (uint32_t)PER) w[0] |= (word_t)pos << (7u * x);
        else w[NW - 1] |= (word_t)pos << (7u * (x - (uint32_t)PER));
    }
    DS2I_DEV uint32_t get(uint32_t x) const {
        if (NW == 1 || x < (uint32_t)PER) return (uint32_t)(w[0] >> (7u * x)) & 127u;
        return (uint32_t)(w[NW - 1] >> (7u * (x - (uint32_t)PER))) & 127u;
    }
};

template <int TMAX>
struct LdsOr { // (the decoded blocks are in dynamic shared memory, see k_disjunctive)
    uint32_t meta[TMAX][M_WORDS];
    uint32_t exc[EXC_LDS_DW]; // + the Simple16 field table (device_codecs.hpp)
    uint32_t st[STAGE_DW];
    uint32_t lord[16];   // list slots by increasing max score
    float lub[16];       // upper_bounds (prefix sums of max scores in that order)
    float wub[16];       // the same prefix sums for the current window: essential lists by their current block's max weight
    uint32_t nomore[16]; // list has no posting >= this doc-id
    uint32_t dupw[TMAX][4]; // bit i of list x: posting i of its current block is owned by an earlier list in this window
};

// MODE 0: top-k (wand / maxscore / ranked_or). MODE 1: or_query (count of the union, queries.hpp:88-131): every list is
// essential, owned candidates are counted. MODE 2: or_query<with_freqs>: additionally every freq of the window is
// summed (the reference touches them all).
// waves per SIMD the top-k instantiations are compiled for: the kernel waits on dependent round trips most of the time, so
// residency is what hides them. <=2 lists: LDS (5.5 KiB per wave) would allow 7; beyond 4 lists LDS caps the residency first
#ifndef DS2I_BLOCKMAX_TMAX
#define DS2I_BLOCKMAX_TMAX 2 // block-max pruning in the top-k union kernels of up to this many lists (see k_disjunctive)
#endif
#ifndef DS2I_DISJ_WAVES2
#define DS2I_DISJ_WAVES2 6
#endif
#ifndef DS2I_DISJ_WAVES4
#define DS2I_DISJ_WAVES4 5
#endif
constexpr int DISJ_WAVES(int tmax, int mode) { return mode != 0 ? 1 : tmax <= 2 ? DS2I_DISJ_WAVES2 : tmax <= 4 ? DS2I_DISJ_WAVES4 : 1; }
template <int TMAX, int CODEC_T, bool STATS = true, int MODE = 0>
__global__ void __launch_bounds__(64, DISJ_WAVES(TMAX, MODE)) DS2I_KN(k_disjunctive)(BatchArgs a) {
    __shared__ LdsOr<TMAX> L;
    // the decoded blocks live in DYNAMIC shared memory, sized by the launch for the longest query it contains
    // (a.dyn_lists <= TMAX list slots: docs[dyn_lists][128] then freqs[dyn_lists][128]). Residency hides this kernel's
    // dependent round trips and LDS per wave caps residency, so a 5-term query should not pay for 8 lists.
    extern __shared__ uint32_t dyn_lds[];
    uint32_t* const Ldocs = dyn_lds;
    uint32_t* const Lfreqs = dyn_lds + 128u * a.dyn_lists;
    const uint32_t lane = lane_id();
    CtxT<CODEC_T, MetaLds, STATS> cx = make_ctx<CODEC_T, MetaLds, STATS>(L, a, Ldocs, Lfreqs);
    for (uint32_t tkt = blockIdx.x; tkt < a.nslice; tkt += gridDim.x) {
        const uint32_t uid = a.order[tkt];
        const unsigned long long t_unit = (STATS && a.unit_clock) ? wall_clock64() : 0ull;
#ifdef DS2I_PHASE_TIMING
        const unsigned long long pt_unit0 = __builtin_readcyclecounter();
#endif
        const Unit u = a.units[uid];
        const uint32_t q = u.q;
        const bool whole = u.nparts == 1;
        const uint32_t N = whole ? a.num_docs : u.blk_end; // the unit's doc-id range is [lo, N)
        uint32_t lo = whole ? 0u : u.blk_begin;
        const uint32_t t0 = a.q_off[q], nt = a.q_off[q + 1] - t0;
        RTopK tk;
        tk.init(a.k);
        unsigned long long count = 0, fsum = 0;
        if (nt == 0 || nt > (uint32_t)TMAX || nt > a.dyn_lists || N == 0) {
            if (whole) {
                if (lane == 0) { a.out_count[q] = 0; if (a.out_freq_sum) a.out_freq_sum[q] = 0; }
                if (MODE == 0) store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
            } else {
                if (lane == 0) { a.unit_count[uid] = 0; a.unit_freq_sum[uid] = 0; }
                if (MODE == 0) store_topk(a.unit_topk, a.unit_topk_len, a.k, uid, tk DS2I_DOCS_ARG(a.unit_topk_docs));
            }
            continue;
        }
        for (uint32_t i = 0; i < nt; ++i) cx.bind(i, a.qterms[t0 + i]);
        if (MODE == 0) cx.s_bytes += 4ull * nt; // max_term_weight[term]
        if (MODE == 0 && a.seed_topk && a.seed_len[q] >= a.k) { // see k_daat: ranked_and's k-th score, relaxed by 1e-5
            const float kth = a.seed_topk[(size_t)q * a.k + a.k - 1];
            tk.floor = __uint_as_float(uniform(__float_as_uint(kth * (1.0f - 1.0e-5f))));
        }
        if (MODE == 0) {
            // static floor (host, from the upload-time block weights): some term of the query has k blocks whose best
            // posting alone scores >= floor1, and a document's score is >= any one of its term scores
            const float f1 = __uint_as_float(uniform(__float_as_uint(a.qterms[t0].floor1))) * (1.0f - 1.0e-5f);
            if (f1 > tk.floor) tk.floor = f1;
        }
        if (lane == 0) {
            for (uint32_t i = 0; i < nt; ++i) { L.lord[i] = i; L.nomore[i] = 0xFFFFFFFFu; }
            for (uint32_t i = 1; i < nt; ++i) { // stable insertion sort by max score (queries.hpp:529-533)
                const uint32_t v = L.lord[i];
                const float kv = __uint_as_float(L.meta[v][M_MAXW]);
                uint32_t j = i;
                while (j > 0 && kv < __uint_as_float(L.meta[L.lord[j - 1]][M_MAXW])) { L.lord[j] = L.lord[j - 1]; --j; }
                L.lord[j] = v;
            }
            float acc = 0.f;
            for (uint32_t i = 0; i < nt; ++i) {
                const float mw = __uint_as_float(L.meta[L.lord[i]][M_MAXW]);
                acc = i ? acc + mw : mw;
                L.lub[i] = acc;
            }
        }
        wave_sync();
        auto ubf = [&](uint32_t i) { return __uint_as_float(uniform(__float_as_uint(L.lub[i]))); };
        auto ubw = [&](uint32_t i) { // this window's bounds (block-max pruning) or the list-level upper_bounds
            return __uint_as_float(uniform(__float_as_uint((MODE == 0 && TMAX <= DS2I_BLOCKMAX_TMAX) ? L.wub[i] : L.lub[i])));
        };
        auto slot_at = [&](uint32_t p) { return uniform(L.lord[p]); };
        auto maxw = [&](uint32_t x) { return __uint_as_float(cx.m(x, M_MAXW)); };
        auto qw = [&](uint32_t x) { return __uint_as_float(cx.m(x, M_QW)); };
        FxScale fx;
        fx.init(ubf(nt - 1));
        uint32_t non_ess = 0;
        auto update_non_ess = [&]() __attribute__((always_inline)) { if (MODE == 0) while (non_ess < nt && !tk.would_enter(ubf(non_ess))) ++non_ess; };
        update_non_ess();
        auto cbw = [&](uint32_t x) { return __uint_as_float(cx.m(x, M_CBW)); }; // q_weight * bmw of the block list x is positioned on
        // POSITIONS list x on the first block whose block_max >= d; false when the list has no posting >= d. With the
        // interleaved skip table the block is only located (table words + its max weight into the list's state) and decoded
        // later, by ensure_docs(), if it can still matter; without it (Elias-Fano layouts) it is decoded at once.
        // `skipping`: the list moves on from its current block after a window that could not hold a result; blocks whose
        // own best posting, added to `rest` (the bound of all the other lists, valid up to doc-id hi2), cannot enter are
        // passed over unexamined (find_block_where).
        // always_inline: left to the inliner, the lambda becomes a real call once it grows, and the call ABI costs this
        // kernel half its throughput
        // block codecs compiled for one codec always come with the table (launch_batch passes it to these kernels
        // unconditionally), so the decode-at-once path is not even compiled into them: one copy less of the decoder
        constexpr bool ALWAYS_TABBED = CODEC_T >= 0 && CODEC_T != CODEC_PEF;
        const bool tabbed = ALWAYS_TABBED || (!cx.is_pef() && cx.skip);
        // Block-max pruning (position first, decode if the block can matter; per-window bounds from the blocks' max weights)
        // pays for queries of <= 2 lists: half the blocks are never decoded. With more lists the sum of the block maxima
        // is rarely below the threshold (measured on the GOV2-scale batch: 3-4 lists decode 6 % fewer blocks, 5+ none) and
        // the bookkeeping costs more than it saves, so those classes keep list-level bounds and decode as they position.
        constexpr bool BLOCKMAX = MODE == 0 && TMAX <= DS2I_BLOCKMAX_TMAX;
        auto position = [&](uint32_t x, uint32_t d, bool may_go_back, bool skipping, float rest, uint32_t hi2, bool eager_freqs) __attribute__((always_inline)) -> bool {
            if (d >= uniform(L.nomore[x])) return false;
            const uint32_t cur = cx.m(x, M_CUR);
            uint32_t from;
            if (cur == 0xFFFFFFFFu) from = 0;
            else if (d > cx.m(x, M_BMAX)) from = cur + 1;
            else if (may_go_back && d < (tabbed ? cx.m(x, M_BASE) : uniform((Ldocs + 128u * x)[0]))) from = 0; // a non-essential list may have been moved ahead
            else return true;
            uint32_t blk, bmax_u;
            float w = 0.f;
            typename decltype(cx)::BlockInfo bi;
            const float* wtab = (BLOCKMAX && a.bmw) ? a.bmw + cx.m(x, M_PBASE) : nullptr;
            {
                PT_BEGIN(cx);
                if (!ALWAYS_TABBED && !tabbed) blk = cx.find_block(x, from, d, bmax_u, wtab, w);
                else if (BLOCKMAX && skipping && wtab) {
                    const float qx = qw(x);
                    blk = cx.find_block_where(x, from, d, bi, wtab, w, [&](uint32_t bm, float wv) { return bm >= hi2 || tk.would_enter((rest + qx * wv) * BOUND_SLACK); });
                } else blk = cx.find_block_info(x, from, d, bi, wtab, w);
                PT_END(cx, PH_FIND);
            }
            if (blk >= cx.m(x, M_NB)) {
                if (lane == 0) L.nomore[x] = d;
                wave_sync();
                return false;
            }
            cx.s_bm_examined += skipping ? blk - from + 1 : 1u;
            cx.s_bytes += 4;
            if (blk != cur) {
                if (BLOCKMAX && tabbed) {
                    cx.setm(x, M_CUR, blk);
                    cx.setm(x, M_BMAX, bi.bmax);
                    cx.setm(x, M_EP, bi.ep);
                    cx.setm(x, M_NEXTEP, bi.next_ep);
                    cx.setm(x, M_BASE, bi.base);
                    cx.setm(x, M_DDEC, 0);
                    cx.setm(x, M_FDEC, 0);
                } else if constexpr (!(BLOCKMAX && ALWAYS_TABBED)) {
                    cx.decode_docs(x, blk, tabbed ? &bi : nullptr);
                    if (MODE == 0 && tabbed) cx.setm(x, M_BASE, bi.base); // (only the lower-list lookups of the top-k modes go back)
                    // the path is bound by dependent round trips, not by instructions: an owner's freqs are wanted for the
                    // freq-only bound of its first candidate, and decoding them now -- while the block's bytes are still
                    // in the staging window -- saves the reload a later decode would wait for
                    if (eager_freqs) cx.decode_freqs(x);
                }
                if (MODE == 0) {
                    cx.setm(x, M_CBW, __float_as_uint(wtab ? qw(x) * w : maxw(x)));
                    wave_sync();
                }
            }
            return true;
        };
        auto ensure_docs = [&](uint32_t x) __attribute__((always_inline)) {
            if constexpr (!BLOCKMAX) return;
            if (cx.m(x, M_DDEC)) return;
            typename decltype(cx)::BlockInfo bi;
            bi.ep = cx.m(x, M_EP);
            bi.next_ep = cx.m(x, M_NEXTEP);
            bi.bmax = cx.m(x, M_BMAX);
            bi.base = cx.m(x, M_BASE);
            cx.decode_docs(x, cx.m(x, M_CUR), &bi);
        };
        // the parts of a split query share a score histogram (ScoreHist). Parts may add a document's term scores in
        // different orders (which lists are essential depends on each part's threshold), hence the 1e-5 relaxation
        const bool shared_floor = MODE == 0 && !whole && a.q_hist;
        ScoreHist sh;
        sh.init(shared_floor ? a.q_hist : nullptr, shared_floor ? a.q_hist_slot[q] : 0u, shared_floor ? ubf(nt - 1) : 0.f, 1.0f - 1.0e-5f);
        ScoreHist::Snapshot hsnap = {0u, 0u, 0u, 0u};
        if (shared_floor) hsnap = sh.load();
        auto adopt_floor = [&]() __attribute__((always_inline)) { // the other parts of this query may have raised the bar
            const float f = sh.floor(hsnap, tk.k);
            hsnap = sh.load(); // resolved a round from now
            if (f > tk.floor) { tk.floor = f; update_non_ess(); }
        };
        uint32_t skip_x = 0xFFFFFFFFu, skip_hi2 = 0; // the list that moves on after a window that was passed over
        float skip_rest = 0.f;
        while (non_ess < nt && lo < N) {
            ++cx.s_rounds;
            // (measured: consulting the histogram every 4th window instead saves the trips and loses as much to the staler floor)
            if (shared_floor) { PT_BEGIN(cx); adopt_floor(); PT_END(cx, PH_FLOOR); }
            if (non_ess >= nt) break;
            // ---- window: every essential list is positioned on its block at lo; [lo, hi] ends with the first of them
#ifdef DS2I_PHASE_TIMING
            const unsigned long long pt_prolog0 = __builtin_readcyclecounter();
#endif
            uint32_t hi = N - 1, hi2 = N - 1, xmin = 0xFFFFFFFFu, live = 0; // live: bit x = essential list x has postings in or after the window
            for (uint32_t p = non_ess; p < nt; ++p) {
                const uint32_t x = slot_at(p);
                if (!position(x, lo, false, x == skip_x, skip_rest, skip_hi2, MODE == 0)) continue;
                live |= 1u << x;
                const uint32_t bm = cx.m(x, M_BMAX);
                if (bm < hi || xmin == 0xFFFFFFFFu) { hi2 = hi; hi = bm < hi ? bm : hi; xmin = x; }
                else if (bm < hi2) hi2 = bm;
                if (!BLOCKMAX && lane < 4) L.dupw[x][lane] = 0; // (block-max windows clear the owners' flags below)
            }
            skip_x = 0xFFFFFFFFu;
            if (!live) break;
            // ---- bounds of this window. wub[p] = the most the lists lord[0..p] can add to a document of the window: the
            // non-essential lists by their list maxima, the essential ones by the max weight of the block they are
            // positioned on (block-max maxscore). The first `ps` lists cannot lift a document into the heap on their own:
            // inside this window they are treated like non-essential lists (looked up for the candidates of the others,
            // decoded only if a candidate needs them); if that is all of them the window is passed over undecoded.
            uint32_t ps = non_ess;
            if constexpr (BLOCKMAX) {
                float acc = 0.f, rest = 0.f;
                ps = nt;
                for (uint32_t p = 0; p < nt; ++p) {
                    const uint32_t x = slot_at(p);
                    const float bnd = p < non_ess ? maxw(x) : (((live >> x) & 1u) ? cbw(x) : 0.f);
                    acc = p ? acc + bnd : bnd;
                    if (x != xmin) rest += bnd;
                    if (lane == 0) L.wub[p] = acc;
                    if (ps == nt && p >= non_ess && tk.would_enter(acc * BOUND_SLACK)) ps = p;
                }
                wave_sync();
                if (ps == nt) { // no document of [lo, hi] can enter: move the list that ends the window, skipping by weight
                    skip_x = xmin;
                    skip_rest = rest;
                    skip_hi2 = hi2;
#ifdef DS2I_PHASE_TIMING
                    cx.s_phase[PH_PROLOG] += __builtin_readcyclecounter() - pt_prolog0;
#endif
                    if (hi == 0xFFFFFFFFu) break;
                    lo = hi + 1;
                    continue;
                }
            }
            if constexpr (BLOCKMAX) {
                for (uint32_t p = ps; p < nt; ++p) {
                    const uint32_t x = slot_at(p);
                    if (!((live >> x) & 1u)) continue;
                    if (!cx.m(x, M_DDEC)) { // docs, then freqs while the block's bytes are in the staging window (see position())
                        ensure_docs(x);
                        cx.decode_freqs(x);
                    }
                    if (lane < 4) L.dupw[x][lane] = 0;
                }
            }
            wave_sync();
#ifdef DS2I_PHASE_TIMING
            cx.s_phase[PH_PROLOG] += __builtin_readcyclecounter() - pt_prolog0;
#endif
            if (MODE == 2) { // every freq of every list inside the window
                unsigned long long fs = 0;
                for (uint32_t p = 0; p < nt; ++p) {
                    const uint32_t x = slot_at(p);
                    if (!((live >> x) & 1u)) continue;
                    const uint32_t c0 = (Ldocs + 128u * x)[lane], c1 = (Ldocs + 128u * x)[lane + 64];
                    const bool i0 = c0 >= lo && c0 <= hi, i1 = c1 >= lo && c1 <= hi;
                    if (!(ballot(i0) | ballot(i1))) continue;
                    if (!cx.m(x, M_FDEC)) cx.decode_freqs(x);
                    fs += (unsigned long long)(i0 ? (Lfreqs + 128u * x)[lane] : 0u) + (i1 ? (Lfreqs + 128u * x)[lane + 64] : 0u);
                }
                for (int o = 32; o; o >>= 1) fs += __shfl_xor(fs, o);
                fsum += fs;
            }
            for (uint32_t p = ps; p < nt; ++p) { // ---- owner list e: its postings in [lo, hi] not owned earlier
                if (p < non_ess) continue;             // became non-essential during this window
                const uint32_t e = slot_at(p);
                if (!((live >> e) & 1u)) continue;
                const uint32_t c0 = (Ldocs + 128u * e)[lane], c1 = (Ldocs + 128u * e)[lane + 64];
                bool v0 = c0 >= lo && c0 <= hi && !((L.dupw[e][lane >> 5] >> (lane & 31u)) & 1u);
                bool v1 = c1 >= lo && c1 <= hi && !((L.dupw[e][2u + (lane >> 5)] >> (lane & 31u)) & 1u);
                if (!(ballot(v0) | ballot(v1))) continue;
                if (MODE != 0) { // or_query: count the owned candidates, mark their copies in the later lists
                    count += (unsigned long long)(__builtin_popcountll(ballot(v0)) + __builtin_popcountll(ballot(v1)));
                    for (uint32_t p2 = p + 1; p2 < nt; ++p2) {
                        const uint32_t x = slot_at(p2);
                        if (!((live >> x) & 1u)) continue;
                        uint32_t q0, q1;
                        if (member_bsearch((Ldocs + 128u * x), c0, v0, q0)) atomicOr(&L.dupw[x][q0 >> 5], 1u << (q0 & 31u));
                        if (member_bsearch((Ldocs + 128u * x), c1, v1, q1)) atomicOr(&L.dupw[x][q1 >> 5], 1u << (q1 & 31u));
                    }
                    wave_sync();
                    continue;
                }
                uint32_t fm0 = 0, fm1 = 0; // lists (beyond e) each candidate occurs in
                PosPack<TMAX> pp0, pp1;   // ... and where
                pp0.clear();
                pp1.clear();
                // lists below the first owner (non-essential, or unable to lift a document of this window): looked up last
                const uint32_t fo = ps > non_ess ? ps : non_ess;
                const float ub_low = fo ? ubw(fo - 1) : 0.f;
                // Range tables (BatchArgs::rmw): what the lower lists can add to THIS candidate, one byte gather per lower
                // list and candidate instead of their list maxima -- and a zero byte says the candidate is not in that list
                // at all, so it is never looked up there. lb*[j] = byte of the list at position j of the max-score order,
                // packed four to a dword.
                constexpr int NL = TMAX - 1, NLW = (NL + 3) / 4;
                const bool use_rmw = MODE == 0 && a.rmw && fo > 0;
                uint32_t lb0[NLW] = {}, lb1[NLW] = {};
                auto low_byte = [&](const uint32_t* lb, uint32_t j) __attribute__((always_inline)) -> uint32_t {
                    uint32_t w = lb[0];
#pragma unroll
                    for (int k = 1; k < NLW; ++k) w = (j >> 2) == (uint32_t)k ? lb[k] : w; // (selects, not a dynamic index: the words stay in registers)
                    return (w >> (8u * (j & 3u))) & 255u;
                };
                // sum of the candidate's bounds in the lower lists at positions <= upto (added from position 0 up)
                auto low_rest = [&](const uint32_t* lb, uint32_t upto) __attribute__((always_inline)) -> float {
                    float r = 0.f;
#pragma unroll
                    for (int j = 0; j < NL; ++j)
                        if ((uint32_t)j <= upto && (uint32_t)j < fo) r = r + __uint_as_float(cx.m(slot_at((uint32_t)j), M_RSCALE)) * (float)low_byte(lb, (uint32_t)j);
                    return r;
                };
                if (use_rmw) {
                    uint32_t e0[NL] = {}, e1[NL] = {};
#pragma unroll
                    for (int j = 0; j < NL; ++j) { // (all gathers are issued before the first is consumed)
                        if ((uint32_t)j < fo) {
                            const uint32_t x = slot_at((uint32_t)j);
                            const uint8_t* tab = a.rmw + 64ull * cx.m(x, M_RBASE);
                            const uint32_t sh = cx.m(x, M_RSHIFT);
                            e0[j] = v0 ? (uint32_t)tab[c0 >> sh] : 0u;
                            e1[j] = v1 ? (uint32_t)tab[c1 >> sh] : 0u;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NL; ++j) {
                        lb0[j >> 2] |= e0[j] << (8 * (j & 3));
                        lb1[j >> 2] |= e1[j] << (8 * (j & 3));
                    }
                }
                // The owner's term score is bounded by its freq alone (doc_term_weight falls with norm_len, so the
                // collection's shortest document bounds it) and by its block's max weight: most postings of a list have
                // small freqs and fall below the threshold here -- before their norm_len is gathered or another list
                // is probed for them.
                if (!cx.m(e, M_FDEC)) cx.decode_freqs(e);
                float pb0, pb1;
                {
                    const float we = qw(e), me = cbw(e);
                    const float fb0 = we * doc_term_weight((Lfreqs + 128u * e)[lane], a.min_norm_len);
                    const float fb1 = we * doc_term_weight((Lfreqs + 128u * e)[lane + 64], a.min_norm_len);
                    pb0 = (fb0 < me ? fb0 : me) + (use_rmw ? low_rest(lb0, fo - 1) : ub_low);
                    pb1 = (fb1 < me ? fb1 : me) + (use_rmw ? low_rest(lb1, fo - 1) : ub_low);
                }
                for (uint32_t p2 = p + 1; p2 < nt; ++p2) {
                    const uint32_t x = slot_at(p2);
                    if (!((live >> x) & 1u)) continue;
                    PT_BEGIN(cx);
                    uint32_t q0, q1;
                    const bool f0 = member_bsearch((Ldocs + 128u * x), c0, v0, q0);
                    const bool f1 = member_bsearch((Ldocs + 128u * x), c1, v1, q1);
                    const float mx = cbw(x);
                    if (f0) { pp0.set(x, q0); atomicOr(&L.dupw[x][q0 >> 5], 1u << (q0 & 31u)); fm0 |= 1u << x; pb0 += mx; }
                    if (f1) { pp1.set(x, q1); atomicOr(&L.dupw[x][q1 >> 5], 1u << (q1 & 31u)); fm1 |= 1u << x; pb1 += mx; }
                    PT_END(cx, PH_MEMBER);
                }
                wave_sync();
                // max-score bound first: nothing below it is gathered, scored or looked up in the lower lists
                bool s0 = v0 && tk.would_enter(pb0 * BOUND_SLACK), s1 = v1 && tk.would_enter(pb1 * BOUND_SLACK);
                uint64_t b0 = ballot(s0), b1 = ballot(s1);
                if (!(b0 | b1)) continue;
                const uint32_t ns = (uint32_t)(__builtin_popcountll(b0) + __builtin_popcountll(b1));
                cx.s_bytes += 4ull * ns;
                cx.s_scored += ns;
                unsigned long long a0 = 0, a1 = 0; // fixed-point sums (FxScale); sc0 / sc1 are their float values
                float sc0 = 0.f, sc1 = 0.f, nl0, nl1;
                {
                    PT_BEGIN(cx);
                    nl0 = s0 ? a.norm_lens[c0] : 0.f;
                    nl1 = s1 ? a.norm_lens[c1] : 0.f;
                    const float w = qw(e);
                    if (s0) a0 = fx.of(w * doc_term_weight((Lfreqs + 128u * e)[lane], nl0));
                    if (s1) a1 = fx.of(w * doc_term_weight((Lfreqs + 128u * e)[lane + 64], nl1));
                    PT_END(cx, PH_SCORE);
                }
                for (uint32_t p2 = p + 1; p2 < nt; ++p2) {
                    const uint32_t x = slot_at(p2);
                    const bool h0 = s0 && ((fm0 >> x) & 1u), h1 = s1 && ((fm1 >> x) & 1u);
                    if (!(ballot(h0) | ballot(h1))) continue;
                    if (!cx.m(x, M_FDEC)) cx.decode_freqs(x);
                    const float w = qw(x);
                    if (h0) a0 += fx.of(w * doc_term_weight((Lfreqs + 128u * x)[pp0.get(x)], nl0));
                    if (h1) a1 += fx.of(w * doc_term_weight((Lfreqs + 128u * x)[pp1.get(x)], nl1));
                }
                // the lower lists, highest bound first; a candidate stops as soon as it cannot enter (queries.hpp:553-564).
                // A list is first only positioned: its block is decoded if some candidate could still enter with the
                // block's best weight on top of its score.
#ifdef DS2I_PHASE_TIMING
                const unsigned long long pt_probe0 = __builtin_readcyclecounter();
#endif
                for (uint32_t p2 = fo; p2-- > 0;) {
                    const float ubp = ubw(p2), lowb = p2 ? ubw(p2 - 1) : 0.f;
                    sc0 = fx.value(a0);
                    sc1 = fx.value(a1);
                    float ubp0 = ubp, ubp1 = ubp, lowb0 = lowb, lowb1 = lowb, own0 = __builtin_inff(), own1 = own0;
                    if (use_rmw) { // per candidate: its own bounds in the lists at positions <= p2, < p2, and in list p2 itself
                        ubp0 = low_rest(lb0, p2);
                        ubp1 = low_rest(lb1, p2);
                        lowb0 = p2 ? low_rest(lb0, p2 - 1) : 0.f;
                        lowb1 = p2 ? low_rest(lb1, p2 - 1) : 0.f;
                        const float sc = __uint_as_float(cx.m(slot_at(p2), M_RSCALE));
                        own0 = sc * (float)low_byte(lb0, p2);
                        own1 = sc * (float)low_byte(lb1, p2);
                    }
                    s0 = s0 && tk.would_enter((sc0 + ubp0) * BOUND_SLACK);
                    s1 = s1 && tk.would_enter((sc1 + ubp1) * BOUND_SLACK);
                    bool r0 = s0, r1 = s1; // still to be looked up in list x
                    if (use_rmw) { // (a zero byte: no posting of the list in the candidate's doc-id range)
                        r0 = r0 && low_byte(lb0, p2) != 0u;
                        r1 = r1 && low_byte(lb1, p2) != 0u;
                    }
                    if (!(ballot(s0) | ballot(s1))) break;
                    if (!(ballot(r0) | ballot(r1))) continue;
                    const uint32_t x = slot_at(p2);
                    for (;;) {
                        const uint64_t rb0 = ballot(r0), rb1 = ballot(r1);
                        if (!(rb0 | rb1)) break;
                        const uint32_t amin = rb0 ? bcast(c0, (uint32_t)__builtin_ctzll(rb0)) : bcast(c1, (uint32_t)__builtin_ctzll(rb1));
                        if (!position(x, amin, true, false, 0.f, 0u, false)) break; // nothing >= amin in list x
                        const uint32_t bm = cx.m(x, M_BMAX);
                        const bool w0 = r0 && c0 <= bm, w1 = r1 && c1 <= bm;
                        bool t0 = w0, t1 = w1;
                        if constexpr (BLOCKMAX) {
                            const float cbx = cbw(x);
                            t0 = w0 && tk.would_enter((sc0 + ((own0 < cbx ? own0 : cbx) + lowb0)) * BOUND_SLACK);
                            t1 = w1 && tk.would_enter((sc1 + ((own1 < cbx ? own1 : cbx) + lowb1)) * BOUND_SLACK);
                        }
                        if (ballot(t0) | ballot(t1)) {
                            ensure_docs(x);
                            uint32_t q0, q1;
                            const bool f0 = member_bsearch((Ldocs + 128u * x), c0, t0, q0);
                            const bool f1 = member_bsearch((Ldocs + 128u * x), c1, t1, q1);
                            if (ballot(f0) | ballot(f1)) {
                                if (!cx.m(x, M_FDEC)) cx.decode_freqs(x);
                                const float w = qw(x);
                                if (f0) a0 += fx.of(w * doc_term_weight((Lfreqs + 128u * x)[q0], nl0));
                                if (f1) a1 += fx.of(w * doc_term_weight((Lfreqs + 128u * x)[q1], nl1));
                            }
                        }
                        s0 = s0 && !(w0 && !t0); // cannot enter even with this block's best posting
                        s1 = s1 && !(w1 && !t1);
                        r0 = r0 && !w0;
                        r1 = r1 && !w1;
                    }
                }
#ifdef DS2I_PHASE_TIMING
                cx.s_phase[PH_PROBE] += __builtin_readcyclecounter() - pt_probe0;
                const unsigned long long pt_ins0 = __builtin_readcyclecounter();
#endif
                sc0 = fx.value(a0);
                sc1 = fx.value(a1);
                bool inserted = false;
                for (int half = 0; half < 2; ++half) {
                    const bool al = half ? s1 : s0;
                    const float sc = half ? sc1 : sc0;
                    uint64_t todo = ballot(al && tk.would_enter(sc));
                    while (todo) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(todo);
                        todo &= todo - 1;
                        const float v = __uint_as_float(bcast(__float_as_uint(sc), src));
                        if (TK_INSERT(tk, v, bcast(half ? c1 : c0, src))) {
                            inserted = true;
                            if (shared_floor && lane == 0) sh.add(v);
                        }
                    }
                }
                if (inserted) update_non_ess(); // queries.hpp:568-574
#ifdef DS2I_PHASE_TIMING
                cx.s_phase[PH_INSERT] += __builtin_readcyclecounter() - pt_ins0;
#endif
            }
            if (hi == 0xFFFFFFFFu) break;
            lo = hi + 1;
        }
        if (whole) {
            if (lane == 0) { a.out_count[q] = MODE == 0 ? tk.n : count; if (a.out_freq_sum) a.out_freq_sum[q] = fsum; }
            if (MODE == 0) store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
        } else {
            if (lane == 0) { a.unit_count[uid] = MODE == 0 ? tk.n : count; a.unit_freq_sum[uid] = fsum; }
            if (MODE == 0) store_topk(a.unit_topk, a.unit_topk_len, a.k, uid, tk DS2I_DOCS_ARG(a.unit_topk_docs));
        }
        if (STATS && a.unit_clock && lane == 0) { a.unit_clock[2ull * uid] = t_unit; a.unit_clock[2ull * uid + 1] = wall_clock64(); }
#ifdef DS2I_PHASE_TIMING
        cx.s_phase[PH_TOTAL] += __builtin_readcyclecounter() - pt_unit0;
#endif
    }
    cx.flush_stats(a.stats);
}

// ------------------------------------------------------------------ top-k of the union as streams (wand / maxscore / ranked_or)
// The three operators return the k best scores of the union of the query's lists (queries.hpp:200-319, 404-476, 478-591);
// what differs in the reference is only how they avoid scoring everything. Here: the lists of a query are ordered by
// decreasing max score, and a document BELONGS to the first list of that order that contains it. A unit streams a block
// range of one list e (its "driver") exactly like ranked_and streams its shortest list -- table window in registers,
// next block prefetched -- and for every posting of the block gathers its range-table byte in every other list:
//   * the lists AFTER e (lower max score) are optional: their bytes bound what they can add, a zero byte says the document
//     is not in that list, so only the few candidates whose bound can enter the heap are ever looked up there;
//   * the lists BEFORE e are exclusions: a candidate found in one of them belongs to that list's units and is dropped
//     (a zero byte settles that without a lookup).
// A document owned by list e occurs in no list of higher max score, so it scores at most S_e = the sum of the max scores
// from e down: once the threshold passes S_e the units of list e -- and of every later list -- end at once. That is
// MaxScore's essential / non-essential split (queries.hpp:529-574), evaluated per unit; no list is walked in lock step
// with another, no window is cut at block boundaries, and every unit is an independent stream for the dispatcher.
// Every document's score is computed by exactly one unit, as the float32 sum of its term scores in the fixed order
// driver, optional lists by decreasing max score: wand == maxscore == ranked_or bit for bit, run after run.
#ifndef DS2I_UT_WAVES2
#define DS2I_UT_WAVES2 6
#endif
constexpr int UT_WAVES(int tmax) { return tmax <= 2 ? DS2I_UT_WAVES2 : tmax <= 4 ? 5 : tmax <= 8 ? 3 : 1; }
template <int TMAX, bool META_IN_LDS, bool WITH_S16>
struct LdsUnionTopk : Lds<TMAX, META_IN_LDS, false, WITH_S16, (TMAX > 2) ? 2 : TMAX> {};

template <int TMAX, int CODEC_T, bool STATS = true>
__global__ void __launch_bounds__(64, UT_WAVES(TMAX)) DS2I_KN(k_union_topk)(BatchArgs a) {
    constexpr bool REG = TMAX <= 4;
    typedef typename std::conditional<REG, MetaReg<TMAX>, MetaLds>::type META;
    __shared__ LdsUnionTopk<TMAX, !REG, CODEC_T != CODEC_PEF && CODEC_T != CODEC_OPTPFOR> L;
    const uint32_t lane = lane_id();
    constexpr bool SHARE_F = TMAX > 2; // one freqs buffer for the driver, one shared by the lists that are looked up
    CtxT<CODEC_T, META, STATS, SHARE_F> cx = make_ctx<CODEC_T, META, STATS, SHARE_F>(L, a);
    cx.want_freqs = cx.side(); // (the driver's freqs with its doc-ids: every posting gets its own bound before any gather)
    const float* const bmw = a.bmw;
    const uint8_t* const rmw = a.rmw;
    constexpr int NW = (TMAX + 3) / 4; // a candidate's bytes, four lists to a dword (byte i = list slot i; slot 0 unused)
    for (uint32_t tkt = blockIdx.x; tkt < a.nslice; tkt += gridDim.x) {
        const uint32_t uid = a.order[tkt];
        const unsigned long long t_unit = (STATS && a.unit_clock) ? wall_clock64() : 0ull;
        const Unit u = a.units[uid];
        const uint32_t vq = u.q;
        const uint32_t q = uniform(a.vq_info[3u * vq]), nexcl = uniform(a.vq_info[3u * vq + 1u]);
        const float s_all = __uint_as_float(uniform(a.vq_info[3u * vq + 2u]));
        const bool whole = u.nparts == 1;
        const uint32_t t0 = a.q_off[vq], nt = a.q_off[vq + 1] - t0;
        RTopK tk;
        tk.init(a.k);
        auto finish_unit = [&]() __attribute__((always_inline)) {
            if (whole) {
                if (lane == 0) a.out_count[q] = tk.n;
                store_topk(a.out_topk, a.out_topk_len, a.k, q, tk DS2I_DOCS_ARG(a.out_topk_docs));
            } else {
                if (lane == 0) { a.unit_count[uid] = tk.n; a.unit_freq_sum[uid] = 0; }
                store_topk(a.unit_topk, a.unit_topk_len, a.k, uid, tk DS2I_DOCS_ARG(a.unit_topk_docs));
            }
            if (STATS && a.unit_clock && lane == 0) { a.unit_clock[2ull * uid] = t_unit; a.unit_clock[2ull * uid + 1] = wall_clock64(); }
        };
        if (nt == 0 || nt > (uint32_t)TMAX) {
            // (an empty query of a k > 64 batch, whose other queries run k_union_stream's big heaps: this heap holds 64 scores, the rest
            // of the query's row is filled here)
            if (whole) for (uint32_t i = 64u + lane; i < a.k; i += 64u) a.out_topk[(size_t)q * a.k + i] = -__builtin_inff();
            finish_unit();
            continue;
        }
        auto bind_one = [&](auto ic) __attribute__((always_inline)) { const uint32_t i = ic; cx.bind(i, a.qterms[t0 + i]); return true; };
        DS2I_LIST_LOOP(0, bind_one)
        cx.s_bytes += 4ull * nt;
        // ---- floors: all lower bounds of the final k-th score of the union
        if (a.seed_topk && a.seed_len[q] >= a.k) { // the ranked_and pass over (a sub-query of) the same query, relaxed for re-association
            const float kth = a.seed_topk[(size_t)q * a.k + a.k - 1];
            tk.floor = __uint_as_float(uniform(__float_as_uint(kth * (1.0f - 1.0e-5f))));
        }
        {   // some term has k blocks whose best posting alone reaches floor1 (host, from the upload-time block weights)
            const float f1 = __uint_as_float(uniform(__float_as_uint(a.qterms[t0].floor1))) * (1.0f - 1.0e-5f);
            if (f1 > tk.floor) tk.floor = f1;
        }
        const bool shared_floor = !whole && a.q_hist;
        ScoreHist sh;
        sh.init(shared_floor ? a.q_hist : nullptr, shared_floor ? a.q_hist_slot[q] : 0u, shared_floor ? s_all : 0.f, 1.0f - 1.0f / 1048576.0f);
        auto adopt_floor = [&]() __attribute__((always_inline)) {
            const float f = sh.floor(tk.k);
            if (f > tk.floor) tk.floor = f;
        };
        if (shared_floor) adopt_floor();
        const float qw0 = __uint_as_float(cx.m(0, M_QW));
        const bool two_trips = TMAX > 2 && a.ut_first && nexcl + a.ut_first + 1u < nt; // (optional lists are left for a second trip)
        // S_e: a document owned by the driver is in no list of higher max score
        const float s_e = __uint_as_float(uniform(__float_as_uint(a.qterms[t0].max_bmw + a.qterms[t0].suf_bmw)));
        if (!tk.would_enter(s_e * BOUND_SLACK)) { finish_unit(); continue; }
        const float* const w0tab = bmw + cx.m(0, M_PBASE);
        // a candidate's bytes: byte (i & 3) of word (i >> 2) = its range-table entry in list slot i
        auto byte_of = [&](const uint32_t* pk, uint32_t i) __attribute__((always_inline)) -> uint32_t {
            uint32_t w = pk[0];
#pragma unroll
            for (int k2 = 1; k2 < NW; ++k2) w = (i >> 2) == (uint32_t)k2 ? pk[k2] : w;
            return (w >> (8u * (i & 3u))) & 255u;
        };
        // what the optional lists after slot `after` can add to the candidate (slots nexcl+1 .. nt-1 are the optional ones)
        auto rest_of = [&](const uint32_t* pk, uint32_t after) __attribute__((always_inline)) -> float {
            float r = 0.f;
            if constexpr (REG) { // (register-resident list state: the slot must be a compile-time constant)
                auto add_one = [&](auto jc) __attribute__((always_inline)) {
                    constexpr uint32_t j = decltype(jc)::value;
                    if (j < nt && j > nexcl && j > after) r = r + __uint_as_float(cx.m(j, M_RSCALE)) * (float)byte_of(pk, j);
                };
                static_loop_down<TMAX, 1>(add_one);
            } else {
                for (uint32_t j = nt; j-- > 1;) {
                    if (j <= nexcl || j <= after) break;
                    r = r + __uint_as_float(cx.m(j, M_RSCALE)) * (float)byte_of(pk, j);
                }
            }
            return r;
        };
        // what the optional lists can add to any document at most (their list maxima, summed like rest_of sums their bytes)
        uint32_t pk_ff[NW];
#pragma unroll
        for (int k2 = 0; k2 < NW; ++k2) pk_ff[k2] = 0xFFFFFFFFu;
        const float opt_all = rest_of(pk_ff, 0);
        // ---- the driver as a stream (see k_conjunctive): table window in registers, next block requested ahead
        const bool pstream = cx.is_pef();
        const uint2* const tab0 = pstream ? nullptr : cx.skip + cx.m(0, M_PBASE);
        const uint32_t* const cmax0 = pstream ? (const uint32_t*)cx.ptr(0, M_MAXS_LO) : nullptr;
        const uint32_t* const ent0 = pstream ? (const uint32_t*)cx.ptr(0, M_END_LO) : nullptr;
        const uint8_t* data0 = nullptr;
        if (!pstream) {
            const uint32_t nb0 = cx.m(0, M_NB);
            data0 = cx.ptr(0, M_MAXS_LO) + 4ull * nb0 + 4ull * (nb0 - 1);
        }
        uint32_t s_first = 0, pf_blk = 0xFFFFFFFFu, pf_d0 = 0, pf_d1 = 0, pf_x = 0;
        uint2 s_e2 = make_uint2(0xFFFFFFFFu, 0u);
        float s_w = 0.f, s_rb = 0.f;
        auto s_fill = [&](uint32_t first) __attribute__((always_inline)) {
            s_first = first;
            const uint32_t idx = first + lane;
            s_e2 = make_uint2(0xFFFFFFFFu, 0u);
            s_w = 0.f;
            if (idx < u.blk_end) {
                if (pstream) s_e2.x = cmax0[idx]; else s_e2 = tab0[idx];
                s_w = w0tab[idx];
            }
            // the optional lists' largest entry over the block's own doc-id span (<= 16 bytes of the level that is wide enough)
            const uint32_t prev_max = (uint32_t)__shfl_up((int)s_e2.x, 1);
            const uint32_t base = (lane == 0) ? 0u : prev_max + 1u, top = s_e2.x;
            const bool row = idx < u.blk_end && (lane > 0 || idx == 0) && top != 0xFFFFFFFFu && base <= top;
            float acc = 0.f;
            auto span_max = [&](uint32_t sh, uint32_t rbase, float scale) __attribute__((always_inline)) {
                const RmwLevels g(a.num_docs, sh);
                const uint8_t* tb = rmw + 64ull * rbase;
                uint32_t best = 255u;
                {   // branch-free (see k_conjunctive): a lane without a row reads entry 0 and discards it
                    const uint32_t b2 = row ? base : 0u, t2 = row ? top : 0u;
                    uint32_t lsh = sh, lvl = 0;
                    while (lvl < 2 && (t2 >> lsh) - (b2 >> lsh) >= 16u) { lsh += 6; ++lvl; }
                    const uint32_t lo2 = b2 >> lsh, hi2 = t2 >> lsh;
                    const bool fits = hi2 - lo2 < 16u;
                    const uint32_t m = max_of_bytes16(tb + g.off[lvl] + (fits ? lo2 : 0u), fits ? hi2 - lo2 + 1u : 1u);
                    if (row && fits) best = m;
                }
                acc = acc + scale * (float)best;
            };
            if constexpr (REG) {
                auto one = [&](auto jc) __attribute__((always_inline)) {
                    constexpr uint32_t j = decltype(jc)::value;
                    if (j < nt && j > nexcl) span_max(cx.m(j, M_RSHIFT), cx.m(j, M_RBASE), __uint_as_float(cx.m(j, M_RSCALE)));
                };
                static_loop_down<TMAX, 1>(one);
            } else {
                for (uint32_t j = nt; j-- > 1;) {
                    if (j <= nexcl) break;
                    span_max(cx.m(j, M_RSHIFT), cx.m(j, M_RBASE), __uint_as_float(cx.m(j, M_RSCALE)));
                }
            }
            s_rb = acc;
        };
        auto s_live = [&](uint32_t from) __attribute__((always_inline)) -> uint64_t {
            const uint32_t idx = s_first + lane;
            bool ok = idx >= from && idx < u.blk_end && (lane > 0 || idx == 0);
            ok = ok && tk.would_enter((qw0 * s_w + s_rb) * BOUND_SLACK);
            return ballot(ok);
        };
        auto s_next = [&](uint32_t from) __attribute__((always_inline)) -> uint32_t {
            for (;;) {
                if (from >= u.blk_end) return u.blk_end;
                const uint64_t hit = s_live(from);
                if (hit) return s_first + (uint32_t)__builtin_ctzll(hit);
                if (s_first + 64 >= u.blk_end) return u.blk_end;
                s_fill(s_first + 63);
                from = from > s_first + 1 ? from : s_first + 1;
            }
        };
        s_fill(u.blk_begin ? u.blk_begin - 1 : 0);
        uint32_t from = u.blk_begin, floor_tick = 1;
        for (;;) {
            ++cx.s_rounds;
            if (from >= u.blk_end) break;
            if (shared_floor && (floor_tick++ & (DS2I_FLOOR_EVERY - 1)) == 0) {
                adopt_floor();
                if (!tk.would_enter(s_e * BOUND_SLACK)) break; // the driver became non-essential
            }
            const uint32_t blk = s_next(from);
            if (blk >= u.blk_end) break;
            from = blk + 1;
            const uint32_t f = blk - s_first, fp = f ? f - 1 : 0;
            const float wblk = qw0 * __uint_as_float(bcast(__float_as_uint(s_w), f));
            const bool staged = pf_blk == blk;
            if (pstream) {
                cx.decode_docs_pef(0, blk, staged ? &pf_d0 : nullptr);
            } else {
                typename decltype(cx)::BlockInfo bi;
                bi.bmax = bcast(s_e2.x, f);
                bi.next_ep = bcast(s_e2.y, f);
                bi.base = blk ? bcast(s_e2.x, fp) + 1u : 0u;
                bi.ep = blk ? bcast(s_e2.y, fp) : 0u;
                if (staged) {
                    const uint8_t* p = data0 + bi.ep;
                    cx.win.gbase = (const uint8_t*)((uintptr_t)p & ~(uintptr_t)3);
                    cx.win.nbytes = 512;
                    cx.win.st[lane] = pf_d0;
                    cx.win.st[lane + 64] = pf_d1;
                    if (cx.side()) { cx.exc[lane] = pf_x; cx.slot_blk = cx.m(0, M_PBASE) + blk; } // (its side slot came with them)
                    wave_sync();
                }
                cx.decode_docs(0, blk, &bi, staged);
            }
            {   // request what the block that is next as things stand will need first
                const uint64_t nx = s_live(blk + 1);
                pf_blk = 0xFFFFFFFFu;
                if (nx) {
                    const uint32_t fn = (uint32_t)__builtin_ctzll(nx);
                    if (pstream) {
                        const uint32_t nb2 = s_first + fn, cm = bcast(s_e2.x, fn);
                        pf_d0 = lane == PC_WORDS ? cm : 0u;
                        if (lane < PC_WORDS) pf_d0 = ent0[(size_t)nb2 * PC_WORDS + lane];
                    } else {
                        const uint32_t* g = (const uint32_t*)((uintptr_t)(data0 + bcast(s_e2.y, fn - 1)) & ~(uintptr_t)3);
                        pf_d0 = g[lane];
                        pf_d1 = g[lane + 64];
                        if (cx.side()) pf_x = cx.xslots[(size_t)XSLOT_DW * (cx.m(0, M_PBASE) + s_first + fn) + lane];
                    }
                    pf_blk = s_first + fn;
                }
            }
            const uint32_t c0 = L.docs[0][lane], c1 = L.docs[0][lane + 64];
            bool al0 = c0 != 0xFFFFFFFFu, al1 = c1 != 0xFFFFFFFFu;
            // block_optpfor through the side slots: the block's freqs came with its doc-ids, so every posting has a bound of its
            // OWN term score (doc_term_weight falls with norm_len: the collection's shortest document bounds it from the freq
            // alone). Only the postings that could enter the heap with that bound + the optional lists' maxima ask the other
            // lists' tables at all -- a gather is a cache line per posting and list, and this operator's were 56 GB per batch --
            // and the tests below use the posting's own bound where they used the block's weight.
            float wb0 = wblk, wb1 = wblk;
            if (cx.side() && cx.m(0, M_FDEC)) {
                const float o0 = qw0 * doc_term_weight(L.freqs[0][lane], a.min_norm_len), o1 = qw0 * doc_term_weight(L.freqs[0][lane + 64], a.min_norm_len);
                wb0 = o0 < wblk ? o0 : wblk;
                wb1 = o1 < wblk ? o1 : wblk;
                al0 = al0 && tk.would_enter((wb0 + opt_all) * BOUND_SLACK);
                al1 = al1 && tk.would_enter((wb1 + opt_all) * BOUND_SLACK);
                if (!(ballot(al0) | ballot(al1))) continue;
            }
            // ---- the candidates' bytes in every other list: one gather per list, all issued before the first is consumed
            uint32_t pk0[NW] = {}, pk1[NW] = {};
            {
                // Two trips when the driver has two or more optional lists: first the exclusion lists and the optional list
                // of highest max score (slots 1 .. split), then -- only for the candidates that can still enter the heap with
                // that list's byte and the LIST maxima of the ones after it -- the rest. The later lists are the long,
                // low-scoring ones: their tables are the ones in which every candidate hits a line of its own.
                uint32_t e0[TMAX] = {}, e1[TMAX] = {};
                const uint32_t split = two_trips ? nexcl + a.ut_first : (uint32_t)TMAX;
                float f0 = 0.f, f1 = 0.f, suf_split = 0.f;
                auto load_first = [&](auto ic) __attribute__((always_inline)) {
                    constexpr uint32_t i = decltype(ic)::value;
                    if (i > split) return true;
                    const uint8_t* tab = rmw + 64ull * cx.m(i, M_RBASE);
                    const uint32_t sh = cx.m(i, M_RSHIFT);
                    e0[i] = al0 ? (uint32_t)tab[c0 >> sh] : 0u;
                    e1[i] = al1 ? (uint32_t)tab[c1 >> sh] : 0u;
                    if (i > nexcl) { // an optional list of the first trip: what its byte says it can add
                        const float sc = __uint_as_float(cx.m(i, M_RSCALE));
                        f0 = f0 + sc * (float)e0[i];
                        f1 = f1 + sc * (float)e1[i];
                        if (i == split) suf_split = __uint_as_float(cx.m(i, M_SUF)); // + the list maxima of the ones after it
                    }
                    return true;
                };
                static_list_loop<1, TMAX>(nt, load_first);
                if (split + 1u < nt) {
                    al0 = al0 && tk.would_enter((wb0 + f0 + suf_split) * BOUND_SLACK);
                    al1 = al1 && tk.would_enter((wb1 + f1 + suf_split) * BOUND_SLACK);
                    auto load_rest = [&](auto ic) __attribute__((always_inline)) {
                        constexpr uint32_t i = decltype(ic)::value;
                        if (i <= split) return true;
                        const uint8_t* tab = rmw + 64ull * cx.m(i, M_RBASE);
                        const uint32_t sh = cx.m(i, M_RSHIFT);
                        e0[i] = al0 ? (uint32_t)tab[c0 >> sh] : 0u;
                        e1[i] = al1 ? (uint32_t)tab[c1 >> sh] : 0u;
                        return true;
                    };
                    static_list_loop<1, TMAX>(nt, load_rest);
                }
                auto pack_one = [&](auto ic) __attribute__((always_inline)) {
                    constexpr uint32_t i = decltype(ic)::value;
                    pk0[i >> 2] |= e0[i] << (8u * (i & 3u));
                    pk1[i >> 2] |= e1[i] << (8u * (i & 3u));
                    return true;
                };
                static_list_loop<1, TMAX>(nt, pack_one);
            }
            float r0 = rest_of(pk0, 0), r1 = rest_of(pk1, 0);
            al0 = al0 && tk.would_enter((wb0 + r0) * BOUND_SLACK);
            al1 = al1 && tk.would_enter((wb1 + r1) * BOUND_SLACK);
            if (!(ballot(al0) | ballot(al1))) continue; // nobody of this block can enter: its freqs stay undecoded
            if (a.rmh) {
                // ---- membership hints (BatchArgs::rmh; block_optpfor indexes): a non-zero byte says SOME posting of list i lies in
                // the candidate's range; where the range holds exactly one posting the hint says at which offset. A candidate
                // elsewhere in that range is not in list i: its byte is cleared -- no lookup there (the most expensive thing this
                // kernel does: a block search and a block decode per list), nothing added to its bound by that list, and for an
                // exclusion list the verdict "not theirs". One more byte per candidate and list, for the survivors of the test above.
                const long long hd = (long long)(a.rmh - a.rmw);
                auto clear_byte = [&](uint32_t* pk, uint32_t i) __attribute__((always_inline)) {
#pragma unroll
                    for (int k2 = 0; k2 < NW; ++k2)
                        if ((i >> 2) == (uint32_t)k2) pk[k2] &= ~(255u << (8u * (i & 3u)));
                };
                auto hint_chunk = [&](auto i0c) __attribute__((always_inline)) { // lists i0 .. i0+3: their loads first, then the tests
                    uint32_t hv0[4], hv1[4];
                    auto ld = [&](auto kc) __attribute__((always_inline)) {
                        constexpr uint32_t k2 = decltype(kc)::value;
                        const uint32_t i = (uint32_t)i0c + k2;
                        hv0[k2] = hv1[k2] = 255u;
                        if (i < nt) {
                            const uint8_t* ht = rmw + 64ull * cx.m(i, M_RBASE) + hd;
                            const uint32_t sh = cx.m(i, M_RSHIFT);
                            if (al0 && sh != 0u && byte_of(pk0, i) != 0u) hv0[k2] = (uint32_t)ht[c0 >> sh]; // (one doc-id per entry: nothing to add)
                            if (al1 && sh != 0u && byte_of(pk1, i) != 0u) hv1[k2] = (uint32_t)ht[c1 >> sh];
                        }
                    };
                    auto ts = [&](auto kc) __attribute__((always_inline)) {
                        constexpr uint32_t k2 = decltype(kc)::value;
                        const uint32_t i = (uint32_t)i0c + k2;
                        if (i < nt) {
                            const uint32_t sh = cx.m(i, M_RSHIFT);
                            if (!((hv0[k2] == 255u) | (hv0[k2] == rmh_code(c0, sh)))) clear_byte(pk0, i);
                            if (!((hv1[k2] == 255u) | (hv1[k2] == rmh_code(c1, sh)))) clear_byte(pk1, i);
                        }
                    };
                    if constexpr (REG) { // (register-resident list state: slots must be compile-time constants)
                        constexpr uint32_t I0 = decltype(i0c)::value;
                        auto ld_c = [&](auto kc) __attribute__((always_inline)) { ld(kc); return true; };
                        (void)ld_c;
                        auto one_ld = [&](auto ic) __attribute__((always_inline)) {
                            constexpr uint32_t i = decltype(ic)::value;
                            const uint8_t* ht = rmw + 64ull * cx.m(i, M_RBASE) + hd;
                            const uint32_t sh = cx.m(i, M_RSHIFT);
                            hv0[i - I0] = (al0 && sh != 0u && byte_of(pk0, i) != 0u) ? (uint32_t)ht[c0 >> sh] : 255u;
                            hv1[i - I0] = (al1 && sh != 0u && byte_of(pk1, i) != 0u) ? (uint32_t)ht[c1 >> sh] : 255u;
                            return true;
                        };
                        static_list_loop<I0, (I0 + 4 < TMAX ? I0 + 4 : TMAX)>(nt, one_ld);
                        auto one_ts = [&](auto ic) __attribute__((always_inline)) {
                            constexpr uint32_t i = decltype(ic)::value;
                            const uint32_t sh = cx.m(i, M_RSHIFT);
                            if (!((hv0[i - I0] == 255u) | (hv0[i - I0] == rmh_code(c0, sh)))) clear_byte(pk0, i);
                            if (!((hv1[i - I0] == 255u) | (hv1[i - I0] == rmh_code(c1, sh)))) clear_byte(pk1, i);
                            return true;
                        };
                        static_list_loop<I0, (I0 + 4 < TMAX ? I0 + 4 : TMAX)>(nt, one_ts);
                    } else {
                        ld(std::integral_constant<uint32_t, 0>{}); ld(std::integral_constant<uint32_t, 1>{});
                        ld(std::integral_constant<uint32_t, 2>{}); ld(std::integral_constant<uint32_t, 3>{});
                        ts(std::integral_constant<uint32_t, 0>{}); ts(std::integral_constant<uint32_t, 1>{});
                        ts(std::integral_constant<uint32_t, 2>{}); ts(std::integral_constant<uint32_t, 3>{});
                    }
                };
                if constexpr (REG) {
                    hint_chunk(std::integral_constant<uint32_t, 1>{});
                } else {
                    for (uint32_t i0 = 1; i0 < nt; i0 += 4) hint_chunk(i0);
                }
                r0 = rest_of(pk0, 0);
                r1 = rest_of(pk1, 0);
                al0 = al0 && tk.would_enter((wb0 + r0) * BOUND_SLACK);
                al1 = al1 && tk.would_enter((wb1 + r1) * BOUND_SLACK);
                if (!(ballot(al0) | ballot(al1))) continue;
            }
            // ---- the driver's own term score: freq-only bound first, then the norm_len gather
            if (!cx.m(0, M_FDEC)) cx.decode_freqs(0);
            const uint32_t f0 = L.freqs[0][lane], f1 = L.freqs[0][lane + 64];
            al0 = al0 && tk.would_enter((qw0 * doc_term_weight(f0, a.min_norm_len) + r0) * BOUND_SLACK);
            al1 = al1 && tk.would_enter((qw0 * doc_term_weight(f1, a.min_norm_len) + r1) * BOUND_SLACK);
            const float nl0 = al0 ? a.norm_lens[c0] : 0.f, nl1 = al1 ? a.norm_lens[c1] : 0.f;
            float pa0 = al0 ? qw0 * doc_term_weight(f0, nl0) : 0.f, pa1 = al1 ? qw0 * doc_term_weight(f1, nl1) : 0.f;
            {
                const uint32_t nv = (uint32_t)(__builtin_popcountll(ballot(al0)) + __builtin_popcountll(ballot(al1)));
                cx.s_bytes += 4ull * nv;
                cx.s_scored += nv;
            }
            al0 = al0 && tk.would_enter((pa0 + r0) * BOUND_SLACK);
            al1 = al1 && tk.would_enter((pa1 + r1) * BOUND_SLACK);
            // ---- the other lists, one after the other: exclusions first (slots 1 .. nexcl), then the optional lists by
            // decreasing max score; a list is consulted only for the candidates whose byte there is not zero
            auto resolve_list = [&](auto ic) __attribute__((always_inline)) -> bool {
                const uint32_t i = ic;
                if (!(ballot(al0) | ballot(al1))) return false;
                const bool excl = i <= nexcl;
                bool n0 = al0 && byte_of(pk0, i) != 0u, n1 = al1 && byte_of(pk1, i) != 0u; // still to be looked up in list i
                const float qw = __uint_as_float(cx.m(i, M_QW));
                for (;;) {
                    const uint64_t b0 = ballot(n0), b1 = ballot(n1);
                    if (!(b0 | b1)) break;
                    const uint32_t amin = b0 ? bcast(c0, (uint32_t)__builtin_ctzll(b0)) : bcast(c1, (uint32_t)__builtin_ctzll(b1));
                    if (cx.m(i, M_CUR) == 0xFFFFFFFFu || amin > cx.m(i, M_BMAX)) {
                        const uint32_t cur = cx.m(i, M_CUR);
                        uint32_t blk2, nbmax = 0;
                        float wdummy = 0.f;
                        typename decltype(cx)::BlockInfo bi;
                        const bool tabbed = !cx.is_pef() && cx.skip;
                        if (tabbed) blk2 = cx.find_block_info(i, cur + 1, amin, bi, nullptr, wdummy);
                        else blk2 = cx.find_block(i, cur + 1, amin, nbmax, nullptr, wdummy);
                        cx.s_bm_examined += 1;
                        cx.s_bytes += 4;
                        if (blk2 >= cx.m(i, M_NB)) break; // the list has nothing at or after amin: nobody left is in it
                        cx.decode_docs(i, blk2, tabbed ? &bi : nullptr);
                    }
                    const uint32_t bm = cx.m(i, M_BMAX);
                    const bool w0 = n0 && c0 <= bm, w1 = n1 && c1 <= bm;
                    uint32_t p0 = 0, p1 = 0;
                    const bool m0 = member_bsearch(L.docs[i], c0, w0, p0), m1 = member_bsearch(L.docs[i], c1, w1, p1);
                    if (excl) { // found in a list of higher max score: the document is that list's
                        al0 = al0 && !m0;
                        al1 = al1 && !m1;
                    } else if (ballot(m0) | ballot(m1)) {
                        if (!cx.freqs_ready(i)) cx.decode_freqs(i);
                        const uint32_t* fr = cx.F(i);
                        if (m0) pa0 = pa0 + qw * doc_term_weight(fr[p0], nl0);
                        if (m1) pa1 = pa1 + qw * doc_term_weight(fr[p1], nl1);
                    }
                    n0 = n0 && !w0;
                    n1 = n1 && !w1;
                }
                if (!excl) { // who cannot reach the heap any more is not looked up in the lists still to come
                    al0 = al0 && tk.would_enter((pa0 + rest_of(pk0, i)) * BOUND_SLACK);
                    al1 = al1 && tk.would_enter((pa1 + rest_of(pk1, i)) * BOUND_SLACK);
                }
                return true;
            };
            DS2I_LIST_LOOP(1, resolve_list)
            // ---- whoever is still alive has its complete score
            for (int half = 0; half < 2; ++half) {
                const bool al = half ? al1 : al0;
                const float sc = half ? pa1 : pa0;
                uint64_t todo = ballot(al && tk.would_enter(sc));
                while (todo) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    const float v = __uint_as_float(bcast(__float_as_uint(sc), src));
                    if (TK_INSERT(tk, v, bcast(half ? c1 : c0, src)) && shared_floor && lane == 0) sh.add(v);
                }
            }
        }
        finish_unit();
    }
    cx.flush_stats(a.stats);
}

// ------------------------------------------------------------------ or_query as a stream
// or_query<with_freqs> (queries.hpp:88-131) returns the size of the union of the query's lists (and touches every freq).
// There is nothing to prune and nothing to rank, so the lists need not be walked in lock step at all: a unit owns a doc-id
// range; it takes the range 32 Ki doc-ids at a time, and for every list decodes the blocks that reach into the current
// piece -- each block once, front to back, whatever the other lists do -- setting one bit per posting in a 4 KiB bitmap
// in LDS (ds_or, no global atomics). The piece's popcount is its part of the union. No list is ever searched for another
// list's documents, no window is cut at a block boundary, and the number of lists is not a template parameter (<= 64
// per query; longer queries keep the one-document-per-step kernel). A block that straddles the end of a piece is decoded
// again for the next piece (one extra decode per list and piece); pieces without any block are never visited, because the
// next piece starts at the first doc-id any list can still hold.
constexpr uint32_t UNION_PIECE = 32768u;   // doc-ids per bitmap (4 KiB)
constexpr uint32_t UNION_MAX_LISTS = 64u;
struct LdsUnion : Lds<1, false> { // (one list slot at a time, its enumerator state in registers: MetaReg<1>)
    uint32_t bits[UNION_PIECE / 32];
    uint32_t nextblk[UNION_MAX_LISTS];  // first block of list i not yet fully behind the stream
    uint32_t nextbase[UNION_MAX_LISTS]; // smallest doc-id that block can still contribute
};
template <bool WITH_FREQS, int CODEC_T, bool STATS = true>
__global__ void __launch_bounds__(64, 5) k_union(BatchArgs a) {
    __shared__ LdsUnion L;
    const uint32_t lane = lane_id();
    CtxT<CODEC_T, MetaReg<1>, STATS> cx = make_ctx<CODEC_T, MetaReg<1>, STATS>(L, a);
    cx.want_freqs = WITH_FREQS; // or_freq reads every freq it passes
    for (uint32_t tkt = blockIdx.x; tkt < a.nslice; tkt += gridDim.x) {
        const uint32_t uid = a.order[tkt];
        const unsigned long long t_unit = (STATS && a.unit_clock) ? wall_clock64() : 0ull;
        const Unit u = a.units[uid];
        const uint32_t q = u.q;
        const bool whole = u.nparts == 1;
        const uint32_t unit_lo = whole ? 0u : u.blk_begin, unit_hi = whole ? a.num_docs : u.blk_end;
        const uint32_t t0 = a.q_off[q], nt = a.q_off[q + 1] - t0;
        unsigned long long count = 0, fsum = 0;
        if (nt && nt <= UNION_MAX_LISTS && unit_lo < unit_hi) {
            // position every list on its first block that reaches into the unit
            for (uint32_t i = 0; i < nt; ++i) {
                if (!WITH_FREQS && a.rmw_bitmaps && RmwLevels::has_bitmap(a.qterms[t0 + i].n, a.num_docs)) { // (served from its bitmap: no block to find)
                    if (lane == 0) { L.nextblk[i] = 0u; L.nextbase[i] = unit_lo; }
                    continue;
                }
                cx.bind(0, a.qterms[t0 + i]);
                uint32_t bmax = 0;
                float w;
                const uint32_t nb = cx.m(0, M_NB);
                const uint32_t blk = unit_lo ? cx.find_block(0, 0, unit_lo, bmax, nullptr, w) : 0u;
                cx.s_bm_examined += 1;
                cx.s_bytes += 4;
                if (lane == 0) {
                    L.nextblk[i] = blk < nb ? blk : 0xFFFFFFFFu;
                    L.nextbase[i] = blk < nb ? unit_lo : 0xFFFFFFFFu;
                }
            }
            wave_sync();
            for (;;) {
                // the piece starts at the first doc-id some list can still hold
                uint32_t mine = 0xFFFFFFFFu;
                for (uint32_t i = lane; i < nt; i += 64) mine = L.nextbase[i] < mine ? L.nextbase[i] : mine;
                const uint32_t lo = bcast(wave_incl_min_scan(mine), 63);
                if (lo >= unit_hi) break;
                const uint32_t hi = unit_hi - lo > UNION_PIECE ? lo + UNION_PIECE : unit_hi; // [lo, hi)
                ++cx.s_rounds;
#pragma unroll
                for (uint32_t k = 0; k < UNION_PIECE / 32 / 64; ++k) L.bits[k * 64 + lane] = 0u;
                wave_sync();
                for (uint32_t i = 0; i < nt; ++i) {
                    if (uniform(L.nextbase[i]) >= hi) continue;
                    // a dense list (>= one document in 64) has its exact bitmap behind its range table: its part of the
                    // piece is 1024 words to OR in, not a hundred blocks to decode
                    const QTerm& qt = a.qterms[t0 + i];
                    const bool from_bitmap = a.rmw_bitmaps && RmwLevels::has_bitmap(qt.n, a.num_docs);
                    if (from_bitmap) {
                        const uint32_t* bm = (const uint32_t*)(a.rmw + 64ull * qt.rmw_off64 + RmwLevels(a.num_docs, qt.rmw_shift).bytes());
                        const uint32_t w0 = lo >> 5, shft = lo & 31u, nbits = hi - lo;
#pragma unroll
                        for (uint32_t k = 0; k < UNION_PIECE / 32 / 64; ++k) {
                            const uint32_t idx = k * 64 + lane;
                            if (32u * idx < nbits) {
                                uint32_t v = __builtin_amdgcn_alignbit(bm[w0 + idx + 1], bm[w0 + idx], shft); // bit j = doc-id lo + 32 idx + j
                                const uint32_t left = nbits - 32u * idx;
                                if (left < 32u) v &= (1u << left) - 1u;
                                L.bits[idx] |= v;
                            }
                        }
                        if constexpr (!WITH_FREQS) {
                            if (lane == 0) L.nextbase[i] = hi < unit_hi ? hi : 0xFFFFFFFFu;
                            wave_sync();
                            continue;
                        }
                        // or_query<true> still reads every freq (queries.hpp:118-120): the list's blocks are walked below, but a
                        // block that lies wholly inside the piece has nothing left to say about doc-ids -- its docs part is
                        // stepped over by its header and only its freqs are decoded (OptPFor full blocks)
                        wave_sync();
                    }
                    cx.bind(0, a.qterms[t0 + i]);
                    const uint32_t nb = cx.m(0, M_NB);
                    uint32_t b = uniform(L.nextblk[i]), base = hi;
                    // block indexes with the skip table: the list's table rows for the next 63 blocks sit in registers (lane j =
                    // row wfirst + j, lane 0 the row before the first block served), and the bytes of block b + 1 are requested
                    // while block b is decoded -- the stream costs no dependent round trip per block
                    const bool tabbed = !cx.is_pef() && cx.skip;
                    const uint2* const tab = tabbed ? cx.skip + cx.m(0, M_PBASE) : nullptr;
                    const uint8_t* const data = tabbed ? cx.ptr(0, M_MAXS_LO) + 4ull * nb + 4ull * (nb - 1) : nullptr;
                    uint32_t wfirst = 0, pf_blk = 0xFFFFFFFFu, pf0 = 0, pf1 = 0, pfx = 0; // (pfx: the block's exception side slot, with its bytes)
                    uint2 we = make_uint2(0xFFFFFFFFu, 0u);
                    auto wfill = [&](uint32_t first) __attribute__((always_inline)) {
                        wfirst = first;
                        we = make_uint2(0xFFFFFFFFu, 0u);
                        if (first + lane < nb) we = tab[first + lane];
                    };
                    if (tabbed && b < nb) wfill(b ? b - 1 : 0);
                    while (b < nb) {
                        bool freqs_only = false;
                        if (tabbed) {
                            if (b - wfirst > 63u) wfill(b - 1);
                            const uint32_t f = b - wfirst, fp = f ? f - 1 : 0;
                            typename decltype(cx)::BlockInfo bi;
                            bi.bmax = bcast(we.x, f);
                            bi.next_ep = bcast(we.y, f);
                            bi.base = b ? bcast(we.x, fp) + 1u : 0u;
                            bi.ep = b ? bcast(we.y, fp) : 0u;
                            if (bi.base >= hi) { base = bi.base; break; } // the block starts behind the piece: not decoded yet
                            const bool staged = pf_blk == b;
                            const uint8_t* const pblk = data + bi.ep;
                            if (staged) {
                                cx.win.gbase = (const uint8_t*)((uintptr_t)pblk & ~(uintptr_t)3);
                                cx.win.nbytes = 512;
                                cx.win.st[lane] = pf0;
                                cx.win.st[lane + 64] = pf1;
                                if (cx.side()) { cx.exc[lane] = pfx; cx.slot_blk = cx.m(0, M_PBASE) + b; }
                                wave_sync();
                            }
                            if constexpr (WITH_FREQS && CODEC_T == CODEC_OPTPFOR)
                                freqs_only = from_bitmap && bi.base >= lo && bi.bmax < hi && (b + 1u) * 128u <= cx.m(0, M_N);
                            if (freqs_only) {
                                if (!staged) {
                                    uint32_t hint = bi.next_ep - bi.ep;
                                    if (hint == 0 || hint > STAGE_DW * 4 - 4) hint = STAGE_DW * 4 - 4;
                                    cx.win.load(pblk, hint);
                                }
                                const uint32_t hdr = uniform(cx.win.rd32(pblk)); // OptPFor header: b | exceptions | Simple16 words
                                const uint32_t hb = hdr >> 26, hew = hdr & 0xFFFFu;
                                const uint32_t docs_bytes = hb >= 32 ? 4u * (1u + 128u) : 4u * (1u + hew + 4u * hb);
                                const uint64_t fo = (uint64_t)(pblk + docs_bytes - cx.arena);
                                cx.setm(0, M_CUR, b);
                                cx.setm(0, M_SIZE, 128u);
                                cx.setm(0, M_BMAX, bi.bmax);
                                cx.setm(0, M_FREQ_LO, (uint32_t)fo);
                                cx.setm(0, M_FREQ_HI, (uint32_t)(fo >> 32));
                                cx.setm(0, M_FDEC, 0);
                                cx.setm(0, M_DDEC, 0);
                                cx.s_bytes += 8; // endpoint + header
                            } else {
                                cx.decode_docs(0, b, &bi, staged);
                            }
                            pf_blk = 0xFFFFFFFFu;
                            if (b + 1 < nb && bi.bmax + 1u < hi) { // the next block reaches into this piece too: request its bytes now
                                const uint32_t* g = (const uint32_t*)((uintptr_t)(data + bi.next_ep) & ~(uintptr_t)3);
                                pf0 = g[lane];
                                pf1 = g[lane + 64];
                                if (cx.side()) pfx = cx.xslots[(size_t)XSLOT_DW * (cx.m(0, M_PBASE) + b + 1u) + lane];
                                pf_blk = b + 1;
                            }
                        } else {
                            cx.decode_docs(0, b);
                        }
                        if (freqs_only) { // (every posting of the block is inside the piece, and its bits are set already)
                            cx.decode_freqs(0);
                            unsigned long long fs = (unsigned long long)L.freqs[0][lane] + L.freqs[0][lane + 64];
                            for (int o = 32; o; o >>= 1) fs += __shfl_xor(fs, o);
                            fsum += fs;
                        } else {
                            const uint32_t d0 = L.docs[0][lane], d1 = L.docs[0][lane + 64];
                            const bool in0 = d0 >= lo && d0 < hi, in1 = d1 >= lo && d1 < hi; // (the padding doc-id 0xFFFFFFFF is never inside)
                            if (!from_bitmap) {
                                if (in0) atomicOr(&L.bits[(d0 - lo) >> 5], 1u << ((d0 - lo) & 31u));
                                if (in1) atomicOr(&L.bits[(d1 - lo) >> 5], 1u << ((d1 - lo) & 31u));
                            }
                            if constexpr (WITH_FREQS) { // or_query<true> reads the freq of every posting it passes (queries.hpp:118-120)
                                if (ballot(in0) | ballot(in1)) {
                                    if (!cx.m(0, M_FDEC)) cx.decode_freqs(0); // (side slots: decode_docs delivered them already)
                                    unsigned long long fs = (unsigned long long)(in0 ? L.freqs[0][lane] : 0u) + (in1 ? L.freqs[0][lane + 64] : 0u);
                                    for (int o = 32; o; o >>= 1) fs += __shfl_xor(fs, o);
                                    fsum += fs;
                                }
                            }
                        }
                        const uint32_t bmax = cx.m(0, M_BMAX);
                        if (bmax >= hi) { base = hi; break; }       // reaches past the piece: taken up again by the next one
                        ++b;
                        base = bmax + 1u;
                        if (base >= hi) break;
                    }
                    if (lane == 0) {
                        L.nextblk[i] = b;
                        L.nextbase[i] = b < nb ? base : 0xFFFFFFFFu;
                    }
                    wave_sync();
                }
                uint32_t pc = 0;
#pragma unroll
                for (uint32_t k = 0; k < UNION_PIECE / 32 / 64; ++k) pc += (uint32_t)__builtin_popcount(L.bits[k * 64 + lane]);
                pc = bcast(wave_incl_scan(pc), 63);
                count += pc;
                wave_sync();
            }
        }
        if (whole) {
            if (lane == 0) { a.out_count[q] = count; if (a.out_freq_sum) a.out_freq_sum[q] = fsum; }
        } else {
            if (lane == 0) { a.unit_count[uid] = count; a.unit_freq_sum[uid] = fsum; }
        }
        if (STATS && a.unit_clock && lane == 0) { a.unit_clock[2ull * uid] = t_unit; a.unit_clock[2ull * uid + 1] = wall_clock64(); }
    }
    cx.flush_stats(a.stats);
}
