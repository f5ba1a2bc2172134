// Shared by the class kernels: per-wave LDS layout, enumerator construction, top-k stores
// (part of kernels.hip -- included inside its anonymous namespace, once per translation unit of the list-count classes; not a
// stand-alone header)

template <int TMAX, bool META_IN_LDS = true, bool WITH_POS = true, bool WITH_S16 = true, int NF = TMAX>
struct Lds {
    uint32_t docs[TMAX][128];
    uint32_t freqs[NF][128]; // NF < TMAX: the lists after list 0 share slot 1 (CtxT SHARE_F)
    uint32_t meta[META_IN_LDS ? TMAX : 1][META_IN_LDS ? M_WORDS : 1];
    // + the Simple16 field table (device_codecs.hpp); kernels compiled for the Elias-Fano layouts never read it and leave
    // it out: 928 B per wave, which takes the 3-4-list ranked kernel from 21 to 24 resident workgroups per CU
    uint32_t exc[WITH_S16 ? EXC_LDS_DW : EXC_DW];
    uint32_t st[STAGE_DW];
    uint8_t pos[WITH_POS ? TMAX : 1][WITH_POS ? 128 : 4]; // match position of candidate c in list i (and_freq; row 0
                            // unused by the conjunctive kernel and reused as ord/ub by the daat kernel)
    DS2I_DEV uint32_t* ord() { return (uint32_t*)&pos[0][0]; }       // daat: ordered_enums [TMAX<=16]
    DS2I_DEV float* ub() { return (float*)&pos[0][64]; }             // maxscore upper_bounds [TMAX<=16]
};

DS2I_DEV void bind_meta(MetaLds& m, uint32_t* lds_meta) { m.p = lds_meta; }
template <int T> DS2I_DEV void bind_meta(MetaReg<T>&, uint32_t*) {}

template <int CODEC_T, class META, bool STATS = true, bool SHARE_F = false, class LDS>
DS2I_DEV CtxT<CODEC_T, META, STATS, SHARE_F> make_ctx(LDS& L, const BatchArgs& a, uint32_t* docs, uint32_t* freqs) {
    CtxT<CODEC_T, META, STATS, SHARE_F> c;
    c.docs = docs;
    c.freqs = freqs;
    bind_meta(c.meta, &L.meta[0][0]);
    c.exc = L.exc;
    if constexpr (CODEC_T != CODEC_PEF && CODEC_T != CODEC_OPTPFOR) s16_table_init(L.exc); // (block_optpfor kernels decode through the side slots)
    c.win.st = L.st;
    c.win.gbase = a.arena;
    c.win.nbytes = 0;
    c.arena = a.arena;
    c.bits0 = a.bits0;
    c.bits1 = a.bits1;
    c.codec = a.codec;
    c.num_docs = a.num_docs;
    c.block_profile = a.block_profile;
    c.skip = (const uint2*)a.skip;
    c.xslots = a.xslots;
    c.xovf = a.xovf;
    c.tails = a.tails;
    c.init_stats();
    return c;
}
template <int CODEC_T, class META, bool STATS = true, bool SHARE_F = false, class LDS>
DS2I_DEV CtxT<CODEC_T, META, STATS, SHARE_F> make_ctx(LDS& L, const BatchArgs& a) {
    return make_ctx<CODEC_T, META, STATS, SHARE_F>(L, a, &L.docs[0][0], &L.freqs[0][0]);
}

template <int NK>
DS2I_DEV void store_topk(float* topk, uint32_t* topk_len, uint32_t k, uint32_t slot, const TopKBig<NK>& tk) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int r = 0; r < NK; ++r)
        if ((uint32_t)r * 64u + lane < k) topk[(size_t)slot * k + (uint32_t)r * 64u + lane] = tk.v[r];
    if (lane == 0) topk_len[slot] = tk.n;
}
DS2I_DEV void store_topk(float* topk, uint32_t* topk_len, uint32_t k, uint32_t slot, const TopK& tk) {
    const uint32_t lane = lane_id();
    if (lane < k) topk[(size_t)slot * k + lane] = tk.v;
    if (lane == 0) topk_len[slot] = tk.n;
}

// (DS2I_OP_TOPK_DOCS) the doc-ids beside the scores: 0xFFFFFFFF past n
template <int NK>
DS2I_DEV void store_topk(float* topk, uint32_t* topk_len, uint32_t k, uint32_t slot, const TopKBigD<NK>& tk, uint32_t* docs) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (int r = 0; r < NK; ++r)
        if ((uint32_t)r * 64u + lane < k) {
            topk[(size_t)slot * k + (uint32_t)r * 64u + lane] = tk.v[r];
            docs[(size_t)slot * k + (uint32_t)r * 64u + lane] = tk.d[r];
        }
    if (lane == 0) topk_len[slot] = tk.n;
}
DS2I_DEV void store_topk(float* topk, uint32_t* topk_len, uint32_t k, uint32_t slot, const TopKD& tk, uint32_t* docs) {
    const uint32_t lane = lane_id();
    if (lane < k) { topk[(size_t)slot * k + lane] = tk.v; docs[(size_t)slot * k + lane] = tk.d; }
    if (lane == 0) topk_len[slot] = tk.n;
}
