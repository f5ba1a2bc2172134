// Plain structs shared by the HIP kernels (*.hip) and the host C-ABI (capi*.cpp): every struct that crosses that boundary is
// defined here, once. The launchers that take them are declared in launchers.hpp.
#pragma once
#include <stdint.h>

namespace ds2i_dev {

// One query term as prepared by the host: byte range of its posting list inside the device
// arena (block indexes) or of its chunk directory (opt index: cmax[] at list_off, 12-dword chunk entries at
// list_end) + BM25 weights (bm25.hpp:17-24 needs logf -> computed on the host).
struct QTerm {
    uint64_t list_off; // byte offset of vbyte(n) in the arena
    uint64_t list_end; // byte offset one past the list
    uint32_t n;        // postings
    float q_weight;
    float max_weight; // q_weight * max_term_weight[term]
    uint32_t term;    // block indexes: term id ; opt index: number of chunks of the list
    uint64_t aux0;    // opt index: absolute bit offset of the list's docs sequence (after its gamma header);
                      // block indexes: number of blocks of all preceding lists (access-profile base)
    uint64_t aux1;    // opt index: absolute bit offset of the list's freqs sequence;
                      // block_optpfor with side tables: dword offset of the list's partial last block in BatchArgs::tails
    uint32_t blk_base; // blocks (chunks) of all preceding lists: index of this list's first entry in bmw[]
    float max_bmw;     // q_weight * (max over the list's blocks of bmw[]): device-computed list bound (ranked_and pruning)
    float suf_bmw;     // sum of max_bmw over the LATER lists of the query (enumerator order)
    float floor1;      // one-term ranked queries: q_weight * (k-th largest bmw of the list) -- k documents reach it
    // doc-id-range max-weight table of the list (rmw, see BatchArgs::rmw): entry (doc >> rmw_shift) of the byte array at
    // rmw + 64 * rmw_off64; rmw_scale * entry bounds q_weight * doc_term_weight of any posting of that doc-id range
    uint32_t rmw_off64;
    uint32_t rmw_shift;
    float rmw_scale;   // q_weight * (list max block weight) / 255
    uint32_t nblocks;  // blocks (block indexes) / chunks (freq_index layouts) of the list
};
static_assert(sizeof(QTerm) == 80, "QTerm is an 80-byte device record");

enum { PH_TOTAL = 0, PH_DOCS, PH_FREQS, PH_FIND, PH_MEMBER, PH_SCORE, PH_TOPK, PH_PROLOG, PH_PROBE, PH_INSERT, PH_STREAM, PH_PREFETCH, PH_FLOOR, PH_UNIT,
       PH_C_VISIT, PH_C_SURV1, PH_C_SURV2, PH_C_BDOCS, PH_C_BFREQS, PH_C_HEAP, PH_C_LIVEROUNDS, PH_C_ALIVE, PH_C_GBLOCKS, /* event counts of the diagnostic build */ PH_COUNT };
struct Stats {
    unsigned long long docs_blocks, freqs_blocks, block_max_examined, algorithmic_bytes, postings_scored, rounds;
    unsigned long long phase_cycles[PH_COUNT]; // summed over waves; only filled with -DDS2I_PHASE_TIMING
};

enum { OP_AND = 0, OP_AND_FREQ = 1, OP_OR = 2, OP_OR_FREQ = 3, OP_RANKED_AND = 4, OP_WAND = 5, OP_MAXSCORE = 6,
       OP_RANKED_OR = 7, OP_REFERENCE_ORDER = 0x100 };

// One schedulable piece of a query: conjunctive queries are split by ranges of blocks of their
// shortest list, the disjunctive operators by doc-id ranges.
struct Unit {
    uint32_t q;         // query id
    uint32_t blk_begin; // first block of list 0 this unit owns
    uint32_t blk_end;   // one past the last block
    uint32_t nparts;    // number of units of query q (1 -> the unit writes the final outputs itself)
};

// k_ranked_stream: everything the start of a unit needs in ONE 32-byte record per ticket of the launch (the unit, its query's
// first term in qterms and its score histogram) -- order[tkt] -> units[uid] -> q_off[q] / q_hist_slot[q] were three dependent
// round trips of a unit that lives for a few dozen blocks
struct UnitRec {
    uint32_t uid, q, blk_begin, blk_end, nparts, qt_off, hist_slot, pad;
};
static_assert(sizeof(UnitRec) == 32, "UnitRec is a 32-byte device record");

struct BatchArgs {
    const uint8_t* arena;     // block indexes: list bytes ; opt index: chunk directory
    const uint8_t* bits0;     // opt index: docs bit vector words
    const uint8_t* bits1;     // opt index: freqs bit vector words
    const float* norm_lens;
    float min_norm_len;       // smallest norm_len of the collection: doc_term_weight(f, min_norm_len) bounds any document's term weight
    const QTerm* qterms;      // terms of all queries, already in enumerator order
    const uint32_t* q_off;    // nq+1 offsets into qterms
    const Unit* units;        // all units, grouped by query
    const uint32_t* order;    // nslice unit ids, scheduling order (costliest first)
    const UnitRec* urec;      // the same order, one record per ticket (ranked conjunctive classes 0 / 1), or null
    uint32_t nslice;
    uint32_t num_docs;
    uint32_t k;
    int codec;
    unsigned long long* unit_clock; // diagnostic (DS2I_UNIT_CLOCK=1, instrumented kernels): {start, end} s_memrealtime of every unit, or null
    unsigned long long* out_count; // nq
    float* out_topk;          // nq*k, descending, padded with -inf
    uint32_t* out_topk_len;   // nq
    unsigned long long* out_freq_sum; // nq (and_freq / or_freq checksum of touched freqs) or null
    uint32_t* out_matches;    // optional doc-id lists (and) or null
    const unsigned long long* match_off; // nq+1 capacity offsets
    // per-unit partial results of split queries (merged by k_merge)
    unsigned long long* unit_count;
    float* unit_topk;         // nunits*k
    uint32_t* unit_topk_len;
    unsigned long long* unit_freq_sum;
    // wand / maxscore: top-k of the ranked_and pass over the same batch. Its k-th score is a valid lower bound of
    // the final k-th score (AND results are a subset of OR results), used as a pruning floor from the first posting
    const float* seed_topk;    // nq*k or null
    const uint32_t* seed_len;  // nq
    // block-synchronous wand / maxscore / ranked_or: the parts of a split query publish their k-th score here (float
    // bits; scores are >= 0 so the bit patterns order like the values) and adopt the maximum as their floor: the final
    // k-th score of the union is >= the k-th score of any part
    unsigned int* q_floor;     // nq or null
    // block-synchronous ranked_and: the parts of a split query share a 256-bucket histogram of the scores that entered
    // their heaps; the lower edge of the highest bucket with >= k documents at or above it is every part's floor
    unsigned int* q_hist;      // (split queries) * 256 or null
    const uint32_t* q_hist_slot; // nq: the query's histogram (rank among the split queries); unused for whole queries
    unsigned int* block_profile; // block indexes: 2 counters per block of the index (docs / freqs decodes) or null
    const void* skip;            // block indexes: interleaved {block_max, block end offset} per block (uint2) or null
    const float* bmw;            // per block / chunk of the index: max doc_term_weight of its postings, or null
    // Doc-id-range max-weight tables (one per list, QTerm::rmw_*), or null: byte e of list t's table covers the doc-ids
    // [e << shift_t, (e + 1) << shift_t); 0 = no posting of the list in that range (=> no document of it can be in an
    // intersection with the list), otherwise an upward-rounded 8-bit quantisation of the largest doc_term_weight in
    // the range relative to the list's maximum. Direct addressing by doc-id: a candidate's bound in every other list
    // costs one byte gather per list and no search (cf. the doc-id-oriented block-max indexes of Dimopoulos, Nepomnyachiy
    // & Suel, WSDM'13). shift_t is chosen per list so that the table holds DS2I_RMW_G..2*DS2I_RMW_G entries per posting.
    // Each table is followed by two coarser levels of itself (level l + 1 entry e = max of level l entries 64 e .. 64 e + 63;
    // every level padded to 64 bytes): the largest entry over the doc-id span of a whole BLOCK of the driving list is found
    // in <= 16 bytes of the level whose entries are wide enough, and bounds every candidate of that block at once.
    const uint8_t* rmw;
    uint32_t rmw_bitmaps;        // the dense lists' exact bitmaps exist behind their tables (RmwLevels::has_bitmap)
    // Membership hints (or null): a second byte per level-1 range-table entry, at the same offsets in a parallel buffer.
    // 0 = the range holds no posting of the list, 255 = it holds two or more, otherwise 1 + (offset of its ONE posting
    // inside the range) mod 254. A candidate whose range holds a single posting at another offset is provably not in the
    // list: for a list with 32 doc-ids per entry that settles 30 of 31 candidates the weight byte lets through, without the
    // block search + block decode a lookup costs (k_ranked_stream; block_optpfor indexes).
    const uint8_t* rmh;
    // Exception side slots (block_optpfor, or null): 64 dwords per block of the index (block b of list t = slot blk_base_t + b)
    // holding the OptPFor exceptions of its docs and freqs parts as position masks + ready-to-OR values (layout:
    // device_codecs.hpp, optpfor_decode_side); xovf = the overflow area of the few blocks whose exceptions do not fit.
    // tails: the partial last block of every list (n % 128 postings; interpolative on disk, serial by construction)
    // expanded to gaps-1 then freqs-1 (+ the byte counts of its two parts), list t's entry at dword aux1_t -- the stream kernels then carry one decoder.
    const uint32_t* xslots;
    const uint32_t* xovf;
    const uint32_t* tails;
    // k_union_topk (wand / maxscore / ranked_or as streams): units belong to VIRTUAL queries = (query, driving list); qterms /
    // q_off then describe the virtual queries, and vq_info holds 3 words per virtual query: the real query, the number
    // of exclusion lists (slots 1 .. nexcl: lists of higher max score -- a document found there is theirs), and the float
    // bits of the real query's score bound (the scale of its shared score histogram). Null for every other kernel.
    const uint32_t* vq_info;
    uint32_t ut_first;    // k_union_topk: optional lists gathered in the first trip (0 = every list in one trip; DS2I_UT_FIRST)
    uint32_t* long_scratch;      // "long" class (> 16 terms): per-unit enumerator state in global memory
    uint32_t long_stride;        // dwords of scratch per unit
    uint32_t dyn_lists;          // union kernels: list slots of decoded blocks in dynamic LDS (>= the longest query of the launch)
    Stats* stats;
    // DS2I_OP_TOPK_DOCS (the *_docs kernels only): the doc-id of every top-k score, same layout as out_topk / unit_topk, 0xFFFFFFFF
    // past the row's length (the seed pass's ids reach the result through k_copy_seed_docs, which takes its own arguments)
    uint32_t* out_topk_docs;
    uint32_t* unit_topk_docs;
};

// What a decode of an index's lists reads, whichever kernel does it (the host fills it in one place: capi_internal.hpp,
// ds2i_index_view; the device makes the decoders' BatchArgs of it in one place: kernels_upload.inc, view_batch_args)
struct IndexView {
    const uint8_t* arena;    // as BatchArgs
    const uint8_t* bits0;
    const uint8_t* bits1;
    int codec;
    uint32_t num_docs;
    const void* skip;        // the side-slot decode (side_decode_block): the interleaved skip table, the slots, their overflow area, the tail table
    const uint32_t* xslots;
    const uint32_t* xovf;
    const uint32_t* tails;
};

// upload-time pass computing bmw[] (k_block_max_weights): one wave per item = <=64 consecutive blocks of one list
struct BmwItem {
    uint32_t list, blk_begin;
};
// geometry of one list's range-table levels, derived from the collection size and the list's shift alone
// membership hint of a doc-id inside its level-1 range (BatchArgs::rmh)
__host__ __device__ inline uint32_t rmh_code(uint32_t doc, uint32_t shift) { return 1u + (doc & ((1u << shift) - 1u)) % 254u; }
struct RmwLevels {
    uint32_t e[3];   // entries of level 1, 2, 3
    uint64_t off[3]; // byte offset of each level from the start of the list's table
    __host__ __device__ RmwLevels(uint32_t num_docs, uint32_t shift) {
        e[0] = (num_docs >> shift) + 1u;
        e[1] = (e[0] + 63u) >> 6;
        e[2] = (e[1] + 63u) >> 6;
        off[0] = 0;
        off[1] = ((uint64_t)e[0] + 63u) & ~63ull;
        off[2] = off[1] + (((uint64_t)e[1] + 63u) & ~63ull);
    }
    __host__ __device__ uint64_t bytes() const { return off[2] + (((uint64_t)e[2] + 63u) & ~63ull); }
    // Lists holding at least one document in 64 additionally get an exact BITMAP of their doc-ids behind the levels (at
    // byte offset bytes(); num_docs bits, padded to 64 bytes + one spare line so that a pair of adjacent words can always
    // be read): <= 64 bits per posting. and_query tests membership in such a list with one bit gather and never decodes
    // it; or_query ORs its words into the union instead of decoding its blocks.
    static __host__ __device__ bool has_bitmap(uint32_t n, uint32_t num_docs) { return (uint64_t)n * 64u >= num_docs; }
    static __host__ __device__ uint64_t bitmap_bytes(uint32_t num_docs) { return ((((uint64_t)num_docs + 31u) / 32u * 4u + 63u) & ~63ull) + 64u; }
    // k_ranked_stream fetches one byte of list 1 ahead for EVERY candidate: the bitmap's instead of the membership hint's where the
    // list has a bitmap and a 128-byte line of it (1024 doc-ids) covers no fewer doc-ids than a line of hints (128 << shift)
    static __host__ __device__ bool bitmap_first(uint32_t n, uint32_t num_docs, uint32_t shift) { return has_bitmap(n, num_docs) && shift <= 3u; }
};
struct BmwArgs {
    IndexView v;
    const float* norm_lens;
    const QTerm* lists; // one per list of the index
    const BmwItem* items;
    uint32_t nitems;
    float* bmw;             // out: one per block
    unsigned int* list_bmw; // out: per list max (float bits; weights are >= 0 so the bit patterns order like the values)
    uint8_t* rmw;           // second pass (k_range_max_weights): the range tables; lists[].max_weight = the list maximum of pass 1
    uint8_t* rmh;           // second pass, level-1 fill: the membership hints (BatchArgs::rmh) or null
    uint32_t bitmaps;       // level-1 pass: also set the bits of the dense lists' bitmaps
    uint32_t rmw_level;     // 0: fill level 1 from the postings; 1 / 2: items = {list, first entry of a 4096-entry run of level
                            // rmw_level + 1}, each entry the maximum of 64 entries of the level below
};

// exception side slot of one block (device_codecs.hpp, optpfor_decode_side): dwords, first add, adds held in-slot, overflow word
// dword 8 / 9: copies of the docs / freqs part's header; dword 10 (XSLOT_FLAG): 0 = the common case -- neither part raw (b < 32),
// both inside the 512 bytes a wave stages from the block's start, every add in the slot -- else bit 31 + (1 + dword offset of
// the block's adds in the overflow area, or 0 when they are in the slot); dwords 11 .. 63: the adds, docs part first
static constexpr uint32_t XSLOT_DW = 64, XSLOT_HDR = 8, XSLOT_FLAG = 10, XSLOT_ADDS = 11, XSLOT_CAP = 53, XSLOT_SLOW = 0x80000000u;

// upload-time pass filling the exception side slots and the tail table (k_build_side_tables): items as in BmwArgs
struct SideArgs {
    const uint8_t* arena;
    const QTerm* lists;
    const BmwItem* items;
    uint32_t nitems;
    uint32_t num_docs;
    const void* skip;          // interleaved skip table
    uint32_t* xslots;          // out: XSLOT_DW dwords per block
    uint32_t* xovf;            // out: overflow area
    unsigned long long xovf_cap; // dwords
    unsigned long long* xovf_cursor; // dwords handed out so far (may run past the capacity: the host then re-runs with more)
    uint32_t* tails;           // out
    unsigned int* bad;         // out: blocks whose header disagrees with their decoded values (corrupt image)
};

// or_query<with_freqs>: the freqs of every posting of every query term, streamed on their own (freq_stream.hip)
struct FreqArgs {
    const uint8_t* arena;
    const void* skip;
    const uint32_t* xslots;
    const uint32_t* xovf;
    const uint32_t* tails;
    const QTerm* qterms;        // the terms of all queries of the batch
    const uint32_t* qterm_q;    // the query each of them belongs to
    unsigned long long* out_freq_sum; // per query: the sum is ADDED (after the union kernels and the merge have written theirs)
};

// and_query / and_query<with_freqs> of queries whose lists are ALL dense enough to carry their exact bitmap (RmwLevels::has_bitmap):
// every list that has to be read is streamed on its own (freq_stream.hip, k_and_stream), membership in the OTHER lists is one bit
// gather per posting and list -- no list is searched, none is decoded for another list's sake
struct StreamTerm {
    uint64_t list_off;   // as QTerm
    uint64_t tail;       // QTerm::aux1: the list's entry of the tail table
    uint32_t n;
    uint32_t blk_base;
    uint32_t q;          // the query the sums belong to
    uint32_t counts;     // 1: this list's matches are the query's result count (its shortest list), 0: freqs only
    uint32_t nother;     // other lists of the query (1..3)
    uint32_t pad;
    uint64_t bm[3];      // byte offsets of their bitmaps from BatchArgs::rmw
};
static_assert(sizeof(StreamTerm) == 64, "StreamTerm is a 64-byte device record");
struct AndStreamArgs {
    const uint8_t* arena;
    const void* skip;
    const uint32_t* xslots;
    const uint32_t* xovf;
    const uint32_t* tails;
    const uint8_t* rmw;
    const StreamTerm* terms;
    unsigned long long* out_count;
    unsigned long long* out_freq_sum; // or null (and_query)
};

struct MergeArgs {
    const uint32_t* split_queries; // ids of queries with nparts > 1
    uint32_t nsplit;
    const uint32_t* q_unit_off;    // nq+1: units of query q are [q_unit_off[q], q_unit_off[q+1])
    uint32_t k;
    int ranked;
    const unsigned long long* unit_count;
    const float* unit_topk;
    const uint32_t* unit_topk_len;
    const unsigned long long* unit_freq_sum;
    unsigned long long* out_count;
    float* out_topk;
    uint32_t* out_topk_len;
    unsigned long long* out_freq_sum;
    const uint32_t* unit_topk_docs; // DS2I_OP_TOPK_DOCS (k_merge_docs / k_merge_big_docs): the parts' doc-ids, and the merged ones
    uint32_t* out_topk_docs;
};

struct DecodeArgs {
    IndexView v;
    QTerm term;
    uint32_t* out_docs;
    uint32_t* out_freqs;
};

// The whole-index walk (walk_index / walk_index_side, kernels_upload.inc): every block (chunk) of the index-wide block numbers
// [block_begin, block_end) -- the blocks of `nlists` consecutive lists, `lists` holding those lists only (their blk_base stay
// index-wide). Block g belongs to the list l with lists[l].blk_base <= g < lists[l].blk_base + lists[l].nblocks; its posting i has
// the place list_first[l] + (position of the block in its list) + i in a collection in CSR form. list_first starts at 0 for the
// first list of the range. The host stages all of it once for every kernel that walks (capi_util.hpp, WalkStaging).
struct WalkArgs {
    IndexView v;
    const QTerm* lists;         // one per list of the range (ds2i_make_qterm)
    uint32_t nlists;
    uint32_t block_begin, block_end;
    const uint64_t* list_first; // nlists + 1 posting offsets
};

// Whole-index decode-and-compare (k_verify_index / k_verify_index_side): the walk over every list of the index against a collection
// staged in CSR form: a posting is compared with exp_docs / exp_freqs at its place.
// The host has compared the list lengths before the launch: list_first[l + 1] - list_first[l] == lists[l].n for every list.
// first_bad receives (atomicMin; preset to VERIFY_NONE) the smallest key (global posting index << 1) | (1: the doc-id matched and
// the freq differs) over all differences -- the first one in (list, position) order, doc-id before freq, whatever the scheduling.
static constexpr unsigned long long VERIFY_NONE = ~0ull;
struct VerifyArgs {
    WalkArgs w;
    const uint32_t* exp_docs;
    const uint32_t* exp_freqs;
    unsigned long long* first_bad;
};

// Whole-index decode-and-store (k_extract_index / k_extract_index_side): the walk over a range of lists; a posting goes to out_docs /
// out_freqs at its place, and the two buffers hold exactly list_first[nlists] postings.
struct ExtractArgs {
    WalkArgs w;
    uint32_t* out_docs;
    uint32_t* out_freqs;
};

// wand / maxscore / ranked_or of a ONE-term query are exactly its ranked_and result: copied from the seed pass (k_copy_seed)
struct CopySeedArgs {
    const uint32_t* queries;
    uint32_t n, k;
    const float* seed_topk;
    const uint32_t* seed_len;
    const unsigned long long* seed_count;
    float* out_topk;
    uint32_t* out_len;
    unsigned long long* out_count;
};
// ... with the doc-ids (DS2I_OP_TOPK_DOCS, k_copy_seed_docs: the seed batch ran the docs kernels too)
struct CopySeedDocsArgs {
    CopySeedArgs s;
    const uint32_t* seed_docs;
    uint32_t* out_docs;
};

// the index encoder and the block_mixed optimiser's plan pass (encode_kernels.hip) over a collection staged in CSR form
struct EncArgs {
    const uint32_t* docs;      // postings of all lists, concatenated
    const uint32_t* freqs;
    const uint64_t* list_in;   // nlists + 1 posting offsets
    const uint32_t* blk_list;  // per block: its list
    const uint32_t* list_blk0; // per list: its first block (global numbering)
    uint32_t nblocks;
    uint8_t* bsel;             // 2 per block: chosen b of the docs / freqs part (full blocks)
    uint32_t* psize;           // 2 per block: bytes of the docs / freqs part
    uint32_t* bmax;            // per block: last doc-id
    const uint64_t* blk_out;   // write pass: byte offset of the block's bytes in `out` (nblocks + 1 entries)
    const uint64_t* list_out;  // write pass: byte offset of the list (its vbyte(n)) in `out`
    uint8_t* out;
    const uint8_t* choice;     // block_mixed write pass: 2 per part (4 per block): mixed type, OptPFor b
    void* rec;                 // optimiser plan: 2 HybRec per block (docs part, freqs part)
};

// What the candidates of one 128-value part cost, as integers -- sizes and counts only: the record k_hybrid_plan fills and the
// optimiser reads (host_hybrid.hpp, where hybrid_part_measure fills the same record on the host)
struct HybRec {
    uint16_t pfor_words[17]; // payload words of OptPFor at OPTPFOR_LOGS[i] (packed values + Simple16 exceptions), 0xFFFF: not a candidate
    uint8_t nexc[17];        // exceptions at that b
    uint8_t interp_ok;       // the values sum to less than 2^32 - 1 (interpolative codes u32 prefix sums)
    uint16_t varint_bytes;
    uint16_t interp_bytes;   // full blocks: valid if interp_ok; partial blocks: the only field that is read
    uint16_t live;           // interpolative tree nodes whose range is not degenerate (interp_live_nodes)
    uint16_t pad[3];
};
static_assert(sizeof(HybRec) == 64, "HybRec is a 64-byte device record");

// The Elias-Fano layouts' encoder (freq_encode_kernels.hip). One FreqJob = one base sequence of one side (docs, or the freqs'
// prefix sums) of one list: a partition of an opt / uniform list, or the whole of an ef / single list -- what seq_write / ef_write
// (host_pef.hpp, host_index.hpp) emit for it. The host sizes and places it (ef_offsets / rb_offsets: closed forms of universe and
// n) and the kernel writes its bits. Offsets are absolute bit positions in the side's bit vector. The jobs of a side are in
// posting order and tile [0, postings): job j holds the postings [src, src + n).
enum : uint32_t { FREQ_SEQ_EF = 0, FREQ_SEQ_RB = 1, FREQ_SEQ_ALL_ONES = 2 }; // host_pef.hpp seq_type
struct FreqJob {
    uint64_t src;      // global index of its first posting
    uint64_t n;
    uint64_t origin;   // stored value of element i: value - origin, and - i more when `shift` (strict Elias-Fano)
    uint64_t type_off; // where the type bit goes (typed: indexed_sequence / strict_sequence)
    uint64_t a_off;    // EF: pointers0        RB: rank1_samples
    uint64_t b_off;    // EF: pointers1        RB: pointers1
    uint64_t hi_off;   // EF: high bits        RB: the characteristic vector
    uint64_t lo_off;   // EF: low bits
    uint64_t hi_len;   // EF: higher_bits_length   RB: universe
    uint64_t na, nb;   // entries of the two sampled arrays
    uint8_t type;      // FREQ_SEQ_*
    uint8_t typed;     // a type bit precedes the sequence
    uint8_t shift;
    uint8_t l;         // EF: lower_bits
    uint8_t wa, wb;    // bits per entry of the two arrays (RB: rank1_sample_size, pointer_size; EF: pointer_size twice)
    uint8_t lsa, lsb;  // log2 of their sampling steps (EF: log_sampling0, log_sampling1; RB: log_rank1_sampling, log_sampling1)
};
static_assert(sizeof(FreqJob) == 96, "FreqJob is a 96-byte device record");

struct FreqEncArgs {
    const uint32_t* docs;     // the side's values: docs (docs side) or cum (freqs side)
    const uint64_t* cum;
    const FreqJob* jobs;
    uint64_t njobs;
    uint64_t postings;
    unsigned long long* out;  // zero-filled, (nbits + 63) / 64 words and two words of padding
    uint64_t nbits;
};

// ---- partition_kernels.hip: the partition DP of the opt layout, one wavefront per (list, side)
// One item's scratch is n + 1 slots of `dist` and of `parent` from `base` on (slot p = "the first p elements are partitioned").
struct PartItem {
    uint32_t list;
    uint32_t side; // 0 = docs (doc-ids over num_docs), 1 = freqs (strict prefix sums over occurrences + 1)
    uint64_t base;
};
constexpr uint32_t PART_MAX_CLASSES = 64; // cost classes are lanes
struct PartArgs {
    const uint32_t* docs;
    const uint64_t* cum;      // per posting: inclusive prefix sum of its list's freqs
    const uint64_t* list_in;  // nlists + 1 posting offsets
    uint64_t nlists;
    uint64_t num_docs;
    const PartItem* items;    // the group's items, longest first
    uint32_t nitems;
    const uint64_t* budget;   // the cost classes' budgets, ascending (computed on the host: the DP's only floating point)
    uint32_t nbudgets;        // <= PART_MAX_CLASSES
    uint64_t fix_cost;
    unsigned long long* dist; // scratch; after the DP an item's end points lie, ascending, in the LAST count u32 of its dist slots
    uint32_t* parent;         // scratch
    uint32_t* count;          // [side * nlists + list]: number of partitions
    const uint64_t* out_offs; // gather: [side * (nlists + 1) + list]: where the list's end points go in out_ends[side]
    uint32_t* out_ends[2];
};

// ---- remap_kernels.hip: doc-ids sent through a doc-id map, and every list sorted again by its new doc-ids with the freqs beside them.
// The host plans the sort from the list lengths (capi_remap.cpp): class 1 lists (<= REMAP_W postings) a wavefront each, class 2
// lists (<= REMAP_L) a workgroup each, the longer ones cut into tiles of at most REMAP_T postings of ONE list, radix-sorted together.
constexpr uint32_t REMAP_W = 64;     // class 1: one posting per lane
constexpr uint32_t REMAP_L = 4096;   // class 2: 8 bytes of LDS per posting, 32 KiB a workgroup (five fit a compute unit's 160 KiB)
constexpr uint32_t REMAP_T = 4096;   // class 3: postings per tile
constexpr uint32_t REMAP_DIGIT = 8;  // class 3: key bits per radix pass
struct RemapTile {
    uint64_t first;   // the tile's first posting
    uint32_t count;   // 1 .. REMAP_T
    uint32_t list3;   // its list, numbered among the class 3 lists
};
struct RemapLong {
    uint64_t first;   // the list's first posting
    uint32_t tile0;   // its first tile
    uint32_t ntiles;
};
struct RemapArgs {
    const uint32_t* doc_map;
    uint64_t num_docs;
    uint64_t postings;
    uint32_t *docs, *freqs;         // the postings as extracted; the map kernel rewrites docs in place
    uint32_t *docs_b, *freqs_b;     // class 3's second buffer pair (null without class 3 lists)
    uint32_t *out_docs, *out_freqs; // where the sorted lists end up: the first pair, or the second when class 3 takes an odd number of passes
    const uint64_t* list_first;     // nlists + 1 posting offsets
    const uint32_t* lists1;         // the class 1 lists
    const uint32_t* lists2;         // the class 2 lists
    uint32_t nlists1, nlists2;
    const RemapTile* tiles;
    const RemapLong* longs;
    uint32_t ntiles, nlongs;
    uint32_t* hist;                 // class 3: (1 << REMAP_DIGIT) words per tile: digit counts, then (after the scan) where each digit's run goes within the list
    uint32_t* flag;                 // set by the map kernel when a doc-id lies outside the map
};

// ---- merge_kernels.hip: the postings of ONE source of a merge stored where the host plan (host_merge.hpp, merge_plan) puts them among
// the merged postings, every doc-id through the source's map or with the source's base added. A wavefront takes a window of
// MERGE_WINDOW consecutive source postings at a time.
constexpr uint32_t MERGE_WINDOW = 1024; // 16 postings a lane
struct MergePlaceArgs {
    const uint32_t *src_docs, *src_freqs; // the source as extracted: `postings` of them
    uint32_t *dst_docs, *dst_freqs;       // the merged postings
    const uint64_t* src_first;            // nlists + 1 posting offsets of the source, from 0
    const uint64_t* dst_first;            // nlists: where each source list's run starts among the merged postings
    const uint32_t* doc_map;              // map_len entries, or null: base + old doc-id
    uint64_t map_len;                     // the source's number of documents
    uint64_t postings;
    uint32_t base;
    uint32_t nlists;                      // >= 1 when there is a posting
    uint32_t* flag;                       // set when a doc-id lies at or past map_len (that posting is not stored)
};

// ---- split_kernels.hip: ONE shard of a split cut out of the source postings. The shard's postings are the stable compaction of the
// source postings by the flag shard_of[doc-id] == shard; the source is cut into windows of SPLIT_WINDOW consecutive postings, a
// wavefront takes a window at a time, and the host scans the windows' counts between the count kernel and the other two.
constexpr uint32_t SPLIT_WINDOW = 1024; // 16 postings a lane
constexpr uint32_t SPLIT_THREADS = 256; // four wavefronts a workgroup
// the workgroups of a launch over `items` wavefronts' worth of work (windows, or list starts): up to 8 a compute unit, which stride
inline unsigned split_grid(uint64_t items, int cus) {
    const uint64_t groups = (items + SPLIT_THREADS / 64 - 1) / (SPLIT_THREADS / 64), cap = 8ull * (uint64_t)(cus > 0 ? cus : 1);
    return (unsigned)(groups < cap ? groups : cap);
}
struct SplitArgs {
    const uint32_t *src_docs, *src_freqs; // the source as extracted: `postings` of them
    uint64_t postings;
    const uint32_t* shard_of;             // num_docs entries; gathered, never read at or past num_docs
    const uint32_t* local;                // num_docs entries: the local id of every document in its shard (scatter)
    uint64_t num_docs;
    uint32_t shard;
    uint64_t nstarts;                     // offsets: the source's nlists + 1 list starts
    uint32_t* win_count;                  // count: the kept postings of every window
    const uint64_t* win_base;             // offsets, scatter: windows + 1 values, the exclusive scan of win_count and its total
    const uint64_t* src_first;            // offsets: nstarts posting offsets of the source, from 0 to `postings`
    uint64_t* kept_before;                // offsets: nstarts values, the shard's postings before every source list start
    uint32_t *dst_docs, *dst_freqs;       // scatter: the shard's postings, win_base[windows] of them
    uint32_t* flag;                       // count: set when a doc-id lies at or past num_docs
};

// ---- invert_kernels.hip: documents (sequences of term ids) inverted into posting lists, and the primitive behind it, the transposition
// of a sparse matrix in CSR form. Both work in windows of INVERT_WINDOW consecutive tokens or entries, a wavefront a window at a time, in
// workgroups of SPLIT_THREADS threads on split_grid's grids.
constexpr uint32_t INVERT_WINDOW = 1024; // 16 tokens a lane
constexpr uint32_t INVERT_DOC_START = 2; // the payload of a document's first token once the mark kernel has run (every other token's is 1)
struct InvertArgs {
    uint32_t *keys, *vals;          // n tokens and their payloads: staged (1), sorted within the documents, marked (INVERT_DOC_START)
    uint64_t n;
    uint64_t nterms;                // stage: a token at or past it raises flag
    const uint64_t* doc_first;      // mark, offsets: ndocs + 1 token offsets, from 0 to n
    uint64_t ndocs;
    uint32_t* win_count;            // count: the run heads of every window
    const uint64_t* win_base;       // offsets, scatter: windows + 1 values, the exclusive scan of win_count and its total
    uint64_t* heads_before;         // offsets: ndocs + 1 values, the entries before every document start
    uint32_t *dst_terms, *dst_freqs; // scatter: win_base[windows] entries; dst_freqs arrives zero-filled
    uint32_t* flag;
};
struct TransposeArgs {
    const uint32_t *cols, *vals;    // n entries in row order
    uint64_t n;
    const uint64_t* row_first;      // nrows + 1 entry offsets, from 0 to n
    uint32_t nrows;                 // >= 1 when there is an entry
    uint64_t ncols;
    uint32_t* count;                // ncols words, zero-filled before either kernel: the histogram (count), the cursors (scatter)
    const uint64_t* col_first;      // scatter: ncols + 1 values, the exclusive scan of the histogram and its total
    uint32_t *out_rows, *out_vals;  // scatter: n entries, column by column, in no order within a column
    uint32_t* flag;                 // count: a column at or past ncols, or a row whose columns do not strictly increase
};

// ---- order_kernels.hip: documents ordered by recursive graph bisection (order_cost.hpp states the arithmetic, host_order.hpp the
// algorithm). The lists lie on the device in p0 order (p0 = a document's position at the level's start), so a term's documents of one
// level segment are one RUN of its list; a run's degrees live at its first entry, its HEAD. Entries are walked in windows of
// ORDER_WINDOW, a wavefront a window at a time; documents and slots a thread each. Workgroups of SPLIT_THREADS threads on
// split_grid's grids.
constexpr uint32_t ORDER_WINDOW = 1024; // 16 entries a lane
struct OrderArgs {
    uint64_t num_docs;              // n
    uint32_t level;                 // l: the segments are level l's, the halves level l + 1's
    const uint32_t* logq;           // n + 3 words: the fixed-point logarithms (host-built)
    uint64_t postings;
    uint32_t* docs;                 // the entries: p0 of every posting, every list in p0 order
    const uint64_t* list_first;     // nlists + 1 entry offsets, from 0 to `postings`
    uint32_t nlists;                // >= 1 when there is a posting
    uint32_t* back;                 // runs: per entry, its distance to its run's head (head = i - back[i])
    uint32_t* run_len;              // runs: at a head, the entries of its run
    uint32_t* deg_right;            // degrees: at a head, the run's documents now in the right half (zero-filled before the launch)
    uint32_t* half_of;              // per position: the level l + 1 segment it lies in (bit 0: the side, the rest: the level l segment)
    uint32_t* side;                 // per p0: the side of the slot the document is in now
    unsigned long long* gain;       // per p0: the sum of its terms' costs, a wrapping int64 (zero-filled before the gains launch)
    uint32_t *keys, *members;       // per slot: the sort key of the member's clamped gain, and the member (a p0)
    const uint32_t* order;          // per position at the level's start: the document there
    uint32_t* next_order;           // compose: order'[s] = order[members[s]]
    uint32_t* inv;                  // compose: inv[members[s]] = s, the map the lists go through at the next level's start
    uint32_t* doc_map;              // finish: doc_map[order[s]] = s
    unsigned long long* exchanges;  // swap: the iteration's exchanges (zeroed before the launch)
    uint32_t* flag;                 // check: a doc-id at or past num_docs
};

// ---- shard_kernels.hip: the top-k rows several shards answered for the same queries merged into the rows of the whole collection
// (include/ds2i_build.h, ds2i_merge_topk, states the key order). One wavefront a workgroup and a query at a time; workgroups stride.
constexpr uint32_t MERGE_TOPK_MAX_ROWS = 64;   // DS2I_HIP_MAX_SHARDS
constexpr uint32_t MERGE_TOPK_MAX_K = 1024;    // DS2I_HIP_MAX_K_LONG: the bitonic network sorts at most that many keys
// k rounded up to a power of two, at least 2: the keys of one LDS buffer
inline uint32_t merge_topk_pow2(uint32_t k) {
    uint32_t p = 2;
    while (p < k) p <<= 1;
    return p;
}
// the workgroups of a launch over nq queries: per compute unit as many as 128 KiB of its LDS hold at 24 * pow2(k) bytes each, at most
// its 32 wavefront slots (5 at k = 1024, 32 from k = 128 down). Sized from the resources alone: no rate was measured at any k.
inline unsigned merge_topk_grid(uint64_t nq, int cus, uint32_t k) {
    const uint64_t fit = (128ull << 10) / (24ull * merge_topk_pow2(k)), per_cu = fit > 32 ? 32 : fit < 1 ? 1 : fit;
    const uint64_t cap = per_cu * (uint64_t)(cus > 0 ? cus : 1);
    return (unsigned)(nq < cap ? nq : cap);
}
struct TopkRowSet {
    const float* scores;            // nq * k
    const uint32_t* docs;           // nq * k, local doc-ids
    const uint32_t* lens;           // nq
    const uint32_t* doc_map;        // map_len collection doc-ids, or null: the ids are the collection's
    uint64_t map_len;
};
struct MergeTopkArgs {
    const TopkRowSet* rows;         // nrows of them, on the device
    uint32_t nrows, nq, k;
    uint32_t pow2;                  // k rounded up to a power of two: the keys of one LDS buffer
    unsigned long long unsorted;    // bit r: row set r's map is not increasing, its rows are sorted by key first
    float* out_scores;              // nq * k
    uint32_t* out_docs;             // nq * k
    uint32_t* out_lens;             // nq
};

} // namespace ds2i_dev
