// List decode, upload-time tables (block-max weights, range tables, hints, side slots), self-tests
// (part of kernels.hip -- included inside its anonymous namespace, once per translation unit of the list-count classes; not a
// stand-alone header)
// ------------------------------------------------------------------ list decode
// The general decoders' BatchArgs of an index view (IndexView, abi_structs.hpp). They read the on-disk bytes: the skip table and the
// side tables of the view stay out (side_decode_block takes those).
DS2I_DEV BatchArgs view_batch_args(const IndexView& v) {
    BatchArgs ba{};
    ba.arena = v.arena;
    ba.bits0 = v.bits0;
    ba.bits1 = v.bits1;
    ba.codec = v.codec;
    ba.num_docs = v.num_docs;
    return ba;
}

// One wave per 128-posting block of ONE list; writes absolute doc-ids and freqs.
__global__ void __launch_bounds__(64) k_decode_list(DecodeArgs a) {
    __shared__ Lds<1> L;
    Ctx cx = make_ctx<-1, MetaLds>(L, view_batch_args(a.v));
    const uint32_t lane = lane_id();
    cx.bind(0, a.term);
    const uint32_t nb = cx.m(0, M_NB);
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        cx.decode_docs(0, b);
        cx.decode_freqs(0);
        const uint32_t sz = cx.m(0, M_SIZE);
        const size_t gpos = cx.m(0, M_GPOS);
        for (uint32_t i = lane; i < sz; i += 64) {
            a.out_docs[gpos + i] = L.docs[0][i];
            a.out_freqs[gpos + i] = L.freqs[0][i];
        }
        wave_sync();
    }
}

// Block b of list t of a block_optpfor index through the exception side slots + tail table (BatchArgs::xslots): the decoder of the
// stream kernels (optpfor_decode_side). Value i of the block's sz postings in lane i & 63: d0 / f0 hold i = lane, d1 / f1
// i = lane + 64 (absolute doc-ids, freqs). st / xs: STAGE_DW / XSLOT_DW dwords of LDS of the wave.
struct SideBlock { uint32_t sz, d0, d1, f0, f1; };
DS2I_DEV SideBlock side_decode_block(const IndexView& v, const QTerm& t, uint32_t b, uint32_t* st, uint32_t* xs) {
    const uint32_t lane = lane_id();
    const uint32_t n = t.n, nb = (n + 127u) >> 7;
    const uint32_t vl = 1u + (n >= (1u << 7)) + (n >= (1u << 14)) + (n >= (1u << 21)) + (n >= (1u << 28));
    const uint8_t* const data = v.arena + t.list_off + vl + 4ull * nb + 4ull * (nb - 1);
    const uint2* const tab = (const uint2*)v.skip + t.blk_base;
    const uint32_t sz = ((b + 1) * 128u <= n) ? 128u : (n & 127u);
    const uint32_t base = b ? tab[b - 1].x + 1u : 0u, ep = b ? tab[b - 1].y : 0u;
    uint32_t v0, v1, f0, f1;
    if (sz == 128u) {
        const uint32_t* const g = (const uint32_t*)(data + ep);
        const uint32_t* const gx = v.xslots + (size_t)XSLOT_DW * (t.blk_base + b);
        st[lane] = g[lane];
        st[lane + 64] = g[lane + 64];
        xs[lane] = gx[lane];
        wave_sync();
        const SlotHead h = optpfor_slot_head(xs);
        if (h.flag == 0u) {
            uint32_t cd, cf;
            optpfor_decode_pair(st, xs, h, v0, v1, f0, f1, cd, cf);
        } else {
            uint32_t nd = 0;
            const uint32_t cons = optpfor_decode_side(st, STAGE_DW, xs, data + ep, v.xovf, 0u, 0u, v0, v1, &nd);
            const uint32_t skip_dw = cons >> 2;
            optpfor_decode_side(st + skip_dw, skip_dw < STAGE_DW ? STAGE_DW - skip_dw : 0u, xs, data + ep + cons, v.xovf, 1u, nd, f0, f1);
        }
    } else {
        const uint32_t* const tl = v.tails + t.aux1;
        v0 = lane < sz ? tl[lane] : 0u;
        v1 = lane + 64 < sz ? tl[lane + 64] : 0u;
        f0 = lane < sz ? tl[sz + lane] : 0u;
        f1 = lane + 64 < sz ? tl[sz + lane + 64] : 0u;
    }
    const uint32_t g0 = (lane < sz) ? v0 + 1u : 0u, g1 = (lane + 64 < sz) ? v1 + 1u : 0u;
    const uint32_t i0 = wave_incl_scan(g0);
    const uint32_t i1 = wave_incl_scan(g1) + bcast(i0, 63);
    return SideBlock{sz, base + i0 - 1u, base + i1 - 1u, f0 + 1u, f1 + 1u};
}

// k_decode_list through the side slots, so that every list-decode test of a block_optpfor index exercises that decoder and the tables
__global__ void __launch_bounds__(64) k_decode_list_side(DecodeArgs a) {
    __shared__ uint32_t st[STAGE_DW];
    __shared__ uint32_t xs[XSLOT_DW];
    const uint32_t lane = lane_id();
    const uint32_t nb = (a.term.n + 127u) >> 7;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const SideBlock k = side_decode_block(a.v, a.term, b, st, xs);
        const size_t gpos = (size_t)b * 128u;
        if (lane < k.sz) { a.out_docs[gpos + lane] = k.d0; a.out_freqs[gpos + lane] = k.f0; }
        if (lane + 64 < k.sz) { a.out_docs[gpos + lane + 64] = k.d1; a.out_freqs[gpos + lane + 64] = k.f1; }
        wave_sync();
    }
}

// ------------------------------------------------------------------ whole-index verification
// Every block (chunk) of every list decoded and compared with a collection staged in CSR form (VerifyArgs, abi_structs.hpp): one
// launch for the whole index, one wave per block, grid-strided over the index-wide block numbers. A wave finds the list of its
// block in the per-list block prefix (QTerm::blk_base / nblocks) by binary search and rebinds only when the list changes
// (walk_index / walk_index_side below, which the extraction kernels share).

// the last list whose blk_base <= g, at or after `lo` (a wave's block numbers only grow; lists[lo].blk_base <= g)
DS2I_DEV uint32_t verify_list_of(const QTerm* lists, uint32_t nlists, uint32_t g, uint32_t lo) {
    uint32_t hi = nlists;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (uniform(lists[mid].blk_base) <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// postings [0, sz) of one decoded block (value i in lane i & 63: d0 / f0 hold i = lane, d1 / f1 i = lane + 64) against the
// collection's postings from `at` on; the block's first difference, if any, is published
DS2I_DEV void verify_compare(const VerifyArgs& a, uint64_t at, uint32_t sz, uint32_t d0, uint32_t d1, uint32_t f0, uint32_t f1) {
    const uint32_t lane = lane_id();
    uint32_t k0 = 0, k1 = 0; // 0: equal, 1: the doc-id differs, 2: the doc-id matches and the freq differs
    if (lane < sz) k0 = d0 != a.exp_docs[at + lane] ? 1u : f0 != a.exp_freqs[at + lane] ? 2u : 0u;
    if (lane + 64 < sz) k1 = d1 != a.exp_docs[at + lane + 64] ? 1u : f1 != a.exp_freqs[at + lane + 64] ? 2u : 0u;
    const uint64_t m0 = ballot(k0 != 0u), m1 = ballot(k1 != 0u);
    if (!(m0 | m1)) return;
    const uint32_t src = (uint32_t)__builtin_ctzll(m0 ? m0 : m1);
    const uint32_t kind = bcast(m0 ? k0 : k1, src);
    const unsigned long long key = ((unsigned long long)(at + src + (m0 ? 0u : 64u)) << 1) | (kind == 2u ? 1ull : 0ull);
    if (lane == 0) atomicMin(a.first_bad, key);
}

// The walk, stated once for the kernels that compare (k_verify_index[_side]) and those that store (k_extract_index[_side]): the wave
// takes the index-wide block numbers blockIdx.x + [a.block_begin, a.block_end) in grid strides, decodes each and hands it to
// sink(at, left, sz, d0, d1, f0, f1): `at` = the block's first posting in the CSR arrays (a.list_first[l] + its position in the
// list), `left` = the postings of its list from that position on, value i of its sz postings in lane i & 63 (d0 / f0: i = lane,
// d1 / f1: i = lane + 64). a.lists holds the lists of the range; their blk_base stay index-wide (WalkArgs, abi_structs.hpp).
template <class Sink>
DS2I_DEV void walk_index(const WalkArgs& a, Lds<1>& L, Sink sink) {
    Ctx cx = make_ctx<-1, MetaLds>(L, view_batch_args(a.v));
    const uint32_t lane = lane_id();
    uint32_t l = 0, n = 0;
    unsigned long long base = 0, end = 0, first = 0; // the bound list: its blocks [base, end) and its first posting in the collection
    for (unsigned long long g = (unsigned long long)a.block_begin + blockIdx.x; g < a.block_end; g += gridDim.x) {
        if (g >= end) {
            l = verify_list_of(a.lists, a.nlists, (uint32_t)g, l);
            const QTerm t = a.lists[l];
            cx.bind(0, t);
            base = t.blk_base;
            end = base + t.nblocks;
            first = a.list_first[l];
            n = t.n;
        }
        cx.decode_docs(0, (uint32_t)(g - base));
        cx.decode_freqs(0);
        const uint32_t gpos = cx.m(0, M_GPOS);
        sink(first + gpos, n > gpos ? n - gpos : 0u, cx.m(0, M_SIZE), L.docs[0][lane], L.docs[0][lane + 64], L.freqs[0][lane], L.freqs[0][lane + 64]);
        wave_sync();
    }
}

// The same through the exception side slots + tail table (side_decode_block, the decode of k_decode_list_side)
template <class Sink>
DS2I_DEV void walk_index_side(const WalkArgs& a, uint32_t* st, uint32_t* xs, Sink sink) {
    uint32_t l = 0;
    unsigned long long base = 0, end = 0, first = 0;
    QTerm t{};
    for (unsigned long long g = (unsigned long long)a.block_begin + blockIdx.x; g < a.block_end; g += gridDim.x) {
        if (g >= end) {
            l = verify_list_of(a.lists, a.nlists, (uint32_t)g, l);
            t = a.lists[l];
            base = t.blk_base;
            end = base + t.nblocks;
            first = a.list_first[l];
        }
        const uint32_t b = (uint32_t)(g - base);
        const SideBlock k = side_decode_block(a.v, t, b, st, xs);
        sink(first + (unsigned long long)b * 128u, t.n - b * 128u, k.sz, k.d0, k.d1, k.f0, k.f1);
        wave_sync();
    }
}

struct VerifySink {
    const VerifyArgs& a;
    DS2I_DEV void operator()(unsigned long long at, uint32_t, uint32_t sz, uint32_t d0, uint32_t d1, uint32_t f0, uint32_t f1) const {
        verify_compare(a, at, sz, d0, d1, f0, f1);
    }
};

__global__ void __launch_bounds__(64) k_verify_index(VerifyArgs a) {
    __shared__ Lds<1> L;
    walk_index(a.w, L, VerifySink{a});
}

__global__ void __launch_bounds__(64) k_verify_index_side(VerifyArgs a) {
    __shared__ uint32_t st[STAGE_DW];
    __shared__ uint32_t xs[XSLOT_DW];
    walk_index_side(a.w, st, xs, VerifySink{a});
}

// ------------------------------------------------------------------ whole-index extraction
// The walk of the verification with stores instead of compares (ExtractArgs, abi_structs.hpp): posting i of a block goes to
// out_docs / out_freqs [at + i] -- two 256-byte rows per side and wave, lane after lane. Lists lie back to back and the buffers have
// no slack: a lane at or past the block's size stores nothing, and no store passes the end of the block's own list whatever the
// decoder says of a block's size.
struct ExtractSink {
    const ExtractArgs& a;
    DS2I_DEV void operator()(unsigned long long at, uint32_t left, uint32_t sz, uint32_t d0, uint32_t d1, uint32_t f0, uint32_t f1) const {
        const uint32_t lane = lane_id();
        sz = sz < left ? sz : left;
        if (lane < sz) { a.out_docs[at + lane] = d0; a.out_freqs[at + lane] = f0; }
        if (lane + 64 < sz) { a.out_docs[at + lane + 64] = d1; a.out_freqs[at + lane + 64] = f1; }
    }
};

__global__ void __launch_bounds__(64) k_extract_index(ExtractArgs a) {
    __shared__ Lds<1> L;
    walk_index(a.w, L, ExtractSink{a});
}

__global__ void __launch_bounds__(64) k_extract_index_side(ExtractArgs a) {
    __shared__ uint32_t st[STAGE_DW];
    __shared__ uint32_t xs[XSLOT_DW];
    walk_index_side(a.w, st, xs, ExtractSink{a});
}

// ------------------------------------------------------------------ upload-time block-max weights
// bmw[block] = max over the block's postings of bm25::doc_term_weight(freq, norm_len[doc]) -- the block-level analogue
// of wand_data's max_term_weight (wand_data.hpp:40-52), with the scoring code's own float32 arithmetic. One wave per
// item = <=64 consecutive blocks of one list: lane j keeps the weight of block blk_begin + j, one coalesced store.
// Range-table entries (BatchArgs::rmw): 0 = no posting in the doc-id range; otherwise 1 + floor(255 * w / list max) capped
// at 255, so that entry * (list max / 255) >= w for every posting of the range (the cap meets w <= list max; the float
// rounding of the two products is far inside the pruning bound's BOUND_SLACK).
DS2I_DEV uint32_t rmw_quantise(float w, float inv) {
    const uint32_t q = (uint32_t)(w * inv) + 1u;
    return q > 255u ? 255u : q;
}
// entry = max(entry, q): bytes have no atomic max, so the containing dword is replaced by compare-and-swap
DS2I_DEV void rmw_raise(uint8_t* tab, uint32_t entry, uint32_t q) {
    unsigned int* word = (unsigned int*)(tab + (entry & ~3u));
    const uint32_t sh = 8u * (entry & 3u);
    unsigned int old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (((old >> sh) & 255u) < q) {
        const unsigned int want = (old & ~(255u << sh)) | (q << sh);
        if (__hip_atomic_compare_exchange_strong(word, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
}

// membership hint of a range: first posting -> its code, any further posting -> 255 (bytes have no atomics: CAS on the dword)
DS2I_DEV void rmh_mark(uint8_t* tab, uint32_t entry, uint32_t code) {
    unsigned int* word = (unsigned int*)(tab + (entry & ~3u));
    const uint32_t sh = 8u * (entry & 3u);
    unsigned int old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t cur = (old >> sh) & 255u;
        if (cur == 255u) break;
        const unsigned int want = (old & ~(255u << sh)) | ((cur ? 255u : code) << sh);
        if (__hip_atomic_compare_exchange_strong(word, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
}

__global__ void __launch_bounds__(64) k_block_max_weights(BmwArgs a) {
    __shared__ Lds<1> L;
    Ctx cx = make_ctx<-1, MetaLds>(L, view_batch_args(a.v));
    const uint32_t lane = lane_id();
    for (uint32_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const BmwItem it = a.items[item];
        const QTerm t = a.lists[it.list];
        if (a.rmw && a.rmw_level) { // coarser levels of the range table: entry e = max of the 64 entries below it
            const RmwLevels g(a.v.num_docs, t.rmw_shift);
            const uint8_t* src = a.rmw + 64ull * t.rmw_off64 + g.off[a.rmw_level - 1];
            uint8_t* dst = a.rmw + 64ull * t.rmw_off64 + g.off[a.rmw_level];
            const uint32_t end = it.blk_begin + 4096u < g.e[a.rmw_level] ? it.blk_begin + 4096u : g.e[a.rmw_level];
            for (uint32_t e = it.blk_begin + lane; e < end; e += 64) { // (every level is zero-padded to 64 bytes: no tail case)
                const uint4* p = (const uint4*)(src + 64ull * e);
                uint32_t m = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint4 v = p[k];
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t x = w[j];
                        uint32_t b = x & 255u, c = (x >> 8) & 255u, d = (x >> 16) & 255u, f = x >> 24;
                        b = b > c ? b : c;
                        d = d > f ? d : f;
                        b = b > d ? b : d;
                        m = m > b ? m : b;
                    }
                }
                dst[e] = (uint8_t)m;
            }
            continue;
        }
        cx.bind(0, t);
        const uint32_t nb = cx.m(0, M_NB);
        const uint32_t end = it.blk_begin + 64u < nb ? it.blk_begin + 64u : nb;
        float mine = 0.f;
        uint8_t* const rtab = a.rmw ? a.rmw + 64ull * t.rmw_off64 : nullptr;
        uint8_t* const htab = (a.rmw && a.rmh) ? a.rmh + 64ull * t.rmw_off64 : nullptr;
        const float rinv = t.max_weight > 0.f ? 255.0f / t.max_weight : 0.f; // second pass: max_weight = the list's largest weight
        unsigned int* const bm = (a.rmw && a.bitmaps && RmwLevels::has_bitmap(t.n, a.v.num_docs))
                                     ? (unsigned int*)(a.rmw + 64ull * t.rmw_off64 + RmwLevels(a.v.num_docs, t.rmw_shift).bytes()) : nullptr;
        for (uint32_t b = it.blk_begin; b < end; ++b) {
            cx.decode_docs(0, b);
            cx.decode_freqs(0);
            const uint32_t sz = cx.m(0, M_SIZE);
            float w = 0.f;
            if (lane < sz) w = doc_term_weight(L.freqs[0][lane], a.norm_lens[L.docs[0][lane]]);
            if (a.rmw && lane < sz) rmw_raise(rtab, L.docs[0][lane] >> t.rmw_shift, rmw_quantise(w, rinv));
            if (htab) {
                if (lane < sz) rmh_mark(htab, L.docs[0][lane] >> t.rmw_shift, rmh_code(L.docs[0][lane], t.rmw_shift));
                if (lane + 64 < sz) rmh_mark(htab, L.docs[0][lane + 64] >> t.rmw_shift, rmh_code(L.docs[0][lane + 64], t.rmw_shift));
            }
            if (bm) { // dense list: its exact bitmap
                if (lane < sz) atomicOr(bm + (L.docs[0][lane] >> 5), 1u << (L.docs[0][lane] & 31u));
                if (lane + 64 < sz) atomicOr(bm + (L.docs[0][lane + 64] >> 5), 1u << (L.docs[0][lane + 64] & 31u));
            }
            if (lane + 64 < sz) {
                const float w1 = doc_term_weight(L.freqs[0][lane + 64], a.norm_lens[L.docs[0][lane + 64]]);
                if (a.rmw) rmw_raise(rtab, L.docs[0][lane + 64] >> t.rmw_shift, rmw_quantise(w1, rinv));
                w = w1 > w ? w1 : w;
            }
            if (a.rmw) { wave_sync(); continue; } // second pass: bmw[] and the list maxima are final already
            for (int o = 32; o; o >>= 1) {
                const float x = __shfl_xor(w, o);
                w = x > w ? x : w;
            }
            if (lane == b - it.blk_begin) mine = w;
            wave_sync();
        }
        if (a.rmw) continue;
        if (it.blk_begin + lane < end) a.bmw[t.blk_base + it.blk_begin + lane] = mine;
        float lm = mine;
        for (int o = 32; o; o >>= 1) {
            const float x = __shfl_xor(lm, o);
            lm = x > lm ? x : lm;
        }
        if (lane == 0) atomicMax(a.list_bmw + it.list, __float_as_uint(lm)); // weights >= 0: bit patterns order like values
    }
}

// ------------------------------------------------------------------ upload-time exception side slots + tail table
// block_optpfor: every full block's OptPFor exceptions, re-stated from its two Simple16 streams as position masks + values
// ready to be OR-ed in (layout: device_codecs.hpp, optpfor_decode_side), and every list's partial last block (interpolative
// on disk) as plain gaps-1 / freqs-1. Both come out of the general decoders, i.e. they hold exactly what a query-time
// decode of the on-disk bytes would produce; the image itself is left as it is. One wave per item = <=64 consecutive
// blocks of one list.
__global__ void __launch_bounds__(64) k_build_side_tables(SideArgs a) {
    __shared__ Lds<1> L;
    BatchArgs ba{};
    ba.arena = a.arena;
    ba.codec = CODEC_OPTPFOR;
    ba.num_docs = a.num_docs;
    ba.skip = a.skip;
    Ctx cx = make_ctx<-1, MetaLds>(L, ba); // (the general decoders: CODEC_OPTPFOR as a template argument means "through the side tables")
    const uint32_t lane = lane_id();
    uint32_t bad = 0;
    for (uint32_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const BmwItem it = a.items[item];
        const QTerm t = a.lists[it.list];
        cx.bind(0, t);
        const uint32_t nb = cx.m(0, M_NB);
        const uint32_t end = it.blk_begin + 64u < nb ? it.blk_begin + 64u : nb;
        const uint2* const tab = (const uint2*)a.skip + t.blk_base;
        const uint8_t* const data = cx.ptr(0, M_MAXS_LO) + 4ull * nb + 4ull * (nb - 1);
        for (uint32_t b = it.blk_begin; b < end; ++b) {
            cx.decode_docs(0, b);
            cx.decode_freqs(0);
            const uint32_t sz = cx.m(0, M_SIZE);
            const uint32_t base = b ? tab[b - 1].x + 1u : 0u, ep = b ? tab[b - 1].y : 0u;
            // gaps - 1 / freqs - 1 as the block decoders deliver them (value i in lane i & 63, slot i >> 6)
            const uint32_t d0 = L.docs[0][lane], d1 = L.docs[0][lane + 64];
            const uint32_t v0 = lane < sz ? (lane ? d0 - L.docs[0][lane - 1] - 1u : d0 - base) : 0u;
            const uint32_t v1 = lane + 64 < sz ? d1 - L.docs[0][lane + 63] - 1u : 0u;
            const uint32_t f0 = lane < sz ? L.freqs[0][lane] - 1u : 0u, f1 = lane + 64 < sz ? L.freqs[0][lane + 64] - 1u : 0u;
            if (sz < 128u) { // the list's partial last block
                uint32_t* const dst = a.tails + t.aux1; // entry: sz gaps-1, sz freqs-1, bytes of the docs part, bytes of the freqs part
                if (lane < sz) { dst[lane] = v0; dst[sz + lane] = f0; }
                if (lane + 64 < sz) { dst[lane + 64] = v1; dst[sz + lane + 64] = f1; }
                const unsigned long long fo = ((unsigned long long)cx.m(0, M_FREQ_HI) << 32) | cx.m(0, M_FREQ_LO);
                if (lane == 0) {
                    dst[2u * sz] = (uint32_t)(fo - (unsigned long long)(data + (b ? tab[b - 1].y : 0u) - a.arena));
                    dst[2u * sz + 1] = (uint32_t)(t.list_end - fo);
                }
                wave_sync();
                continue;
            }
            const uint8_t* const pd = data + ep;
            const uint8_t* const pf = cx.ptr(0, M_FREQ_LO);
            const uint32_t hd = uniform(ld32(pd)), hf = uniform(ld32(pf));
            const uint32_t bd = hd >> 26, bf = hf >> 26;
            const uint32_t keepd = bd < 32u ? ~((1u << bd) - 1u) : 0u, keepf = bf < 32u ? ~((1u << bf) - 1u) : 0u;
            const uint32_t a0 = v0 & keepd, a1 = v1 & keepd, g0 = f0 & keepf, g1 = f1 & keepf;
            const uint64_t md0 = ballot(a0 != 0u), md1 = ballot(a1 != 0u), mf0 = ballot(g0 != 0u), mf1 = ballot(g1 != 0u);
            const uint32_t nd = (uint32_t)(__builtin_popcountll(md0) + __builtin_popcountll(md1));
            const uint32_t nf = (uint32_t)(__builtin_popcountll(mf0) + __builtin_popcountll(mf1));
            if ((bd < 32u && nd != ((hd >> 16) & 0x3FFu)) || (bf < 32u && nf != ((hf >> 16) & 0x3FFu))) ++bad; // (corrupt image)
            uint32_t* const slot = a.xslots + (size_t)XSLOT_DW * (t.blk_base + b);
            uint32_t* dst = slot + XSLOT_ADDS;
            uint32_t ovf = 0;
            bool ok = true;
            // the common case a wave decodes without a branch: neither part raw, both (and the dword a lane may read past the freqs
            // part) inside the 128 dwords staged from the block's start, every add in the slot
            const uint32_t tot_d = 1u + (hd & 0xFFFFu) + 4u * bd, tot_f = 1u + (hf & 0xFFFFu) + 4u * bf;
            const bool common = bd < 32u && bf < 32u && tot_d + tot_f + 1u <= STAGE_DW && nd + nf <= XSLOT_CAP;
            if (nd + nf > XSLOT_CAP) {
                unsigned long long off = 0;
                if (lane == 0) off = atomicAdd(a.xovf_cursor, (unsigned long long)(nd + nf));
                off = ((unsigned long long)bcast((uint32_t)(off >> 32), 0) << 32) | bcast((uint32_t)off, 0);
                ok = off + nd + nf <= a.xovf_cap && off + nd + nf < 0x7FFFFFFFull; // (otherwise the host re-runs the pass with the room the cursor asks for; bit 31 of the slot's offset word is XSLOT_SLOW)
                dst = a.xovf + off;
                ovf = (uint32_t)off + 1u;
            }
            const uint32_t words[8] = {(uint32_t)md0, (uint32_t)(md0 >> 32), (uint32_t)md1, (uint32_t)(md1 >> 32),
                                       (uint32_t)mf0, (uint32_t)(mf0 >> 32), (uint32_t)mf1, (uint32_t)(mf1 >> 32)};
            uint32_t mine = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) mine = lane == (uint32_t)i ? words[i] : mine;
            mine = lane == XSLOT_HDR ? hd : lane == XSLOT_HDR + 1 ? hf : lane == XSLOT_FLAG ? (common ? 0u : (XSLOT_SLOW | (ok ? ovf : 0u))) : mine;
            if (lane <= XSLOT_FLAG) slot[lane] = mine;
            if (ok) {
                const uint32_t r0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(md0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)md0, 0u));
                const uint32_t r1 = (uint32_t)__builtin_popcountll(md0) + __builtin_amdgcn_mbcnt_hi((uint32_t)(md1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)md1, 0u));
                const uint32_t s0 = nd + __builtin_amdgcn_mbcnt_hi((uint32_t)(mf0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mf0, 0u));
                const uint32_t s1 = nd + (uint32_t)__builtin_popcountll(mf0) + __builtin_amdgcn_mbcnt_hi((uint32_t)(mf1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mf1, 0u));
                if (a0) dst[r0] = a0;
                if (a1) dst[r1] = a1;
                if (g0) dst[s0] = g0;
                if (g1) dst[s1] = g1;
            }
            wave_sync();
        }
    }
    if (bad && lane == 0) atomicAdd(a.bad, bad);
}

// top[list][0..63] = the 64 largest bmw values of the list, descending, padded with 0 (one wave per list)
__global__ void __launch_bounds__(64) k_list_top_bmw(const float* bmw, const QTerm* lists, uint32_t nlists, float* top) {
    const uint32_t lane = lane_id();
    for (uint32_t l = blockIdx.x; l < nlists; l += gridDim.x) {
        const QTerm t = lists[l];
        const uint32_t nb = t.nblocks;
        const float* w = bmw + t.blk_base;
        TopK tk;
        tk.init(64);
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const float v = b0 + lane < nb ? w[b0 + lane] : -1.f;
            uint64_t todo = ballot(b0 + lane < nb && tk.would_enter(v));
            while (todo) {
                const uint32_t src = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                tk.insert(__uint_as_float(bcast(__float_as_uint(v), src)));
            }
        }
        top[(size_t)l * 64 + lane] = lane < tk.n ? tk.v : 0.f;
    }
}

// ------------------------------------------------------------------ primitive self-test
__global__ void __launch_bounds__(64) k_selftest(const uint32_t* in, uint32_t* out) {
    const uint32_t lane = lane_id();
    uint32_t x = in[blockIdx.x * 64 + lane];
    out[blockIdx.x * 64 + lane] = wave_incl_scan(x);
}

__global__ void __launch_bounds__(64) k_selftest_bm25(const uint32_t* freqs, const float* norm_lens, float* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + lane_id();
    if (i < n) out[i] = doc_term_weight(freqs[i], norm_lens[i]);
}

// wand / maxscore / ranked_or of a ONE-term query are exactly its ranked_and result: copy it from the seed pass
__global__ void __launch_bounds__(64) k_copy_seed(CopySeedArgs a) {
    const uint32_t lane = lane_id();
    for (uint32_t w = blockIdx.x; w < a.n; w += gridDim.x) {
        const uint32_t q = a.queries[w];
        for (uint32_t i = lane; i < a.k; i += 64) a.out_topk[(size_t)q * a.k + i] = a.seed_topk[(size_t)q * a.k + i]; // (k may exceed one score per lane)
        if (lane == 0) { a.out_len[q] = a.seed_len[q]; a.out_count[q] = a.seed_count[q]; }
    }
}

#ifdef DS2I_DOCS_TU
// ... with the doc-ids (DS2I_OP_TOPK_DOCS: the seed batch ran the docs kernels too)
__global__ void __launch_bounds__(64) k_copy_seed_docs(CopySeedDocsArgs a) {
    const uint32_t lane = lane_id();
    for (uint32_t w = blockIdx.x; w < a.s.n; w += gridDim.x) {
        const uint32_t q = a.s.queries[w];
        for (uint32_t i = lane; i < a.s.k; i += 64) {
            a.s.out_topk[(size_t)q * a.s.k + i] = a.s.seed_topk[(size_t)q * a.s.k + i];
            a.out_docs[(size_t)q * a.s.k + i] = a.seed_docs[(size_t)q * a.s.k + i];
        }
        if (lane == 0) { a.s.out_len[q] = a.s.seed_len[q]; a.s.out_count[q] = a.s.seed_count[q]; }
    }
}
#endif

// FETCH_SIZE calibration (MI355X_MICROARCH.md §HBM): streams `ndw` dwords of the arena with the same
// access shape as Window::load (one dword per lane, 64 consecutive lanes) and folds them into a checksum.
__global__ void __launch_bounds__(64) k_calib_read(const uint32_t* base, unsigned long long ndw, uint32_t* out) {
    uint32_t acc = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 64 + lane_id(); i < ndw;
         i += (unsigned long long)gridDim.x * 64)
        acc ^= base[i];
    for (int o = 32; o; o >>= 1) acc ^= __shfl_xor(acc, o);
    if (lane_id() == 0 && acc == 0x12345678u) out[0] = acc; // keep the loads alive
}
