// The one declaration of every launcher: the functions through which the host translation units (capi*.cpp) start the kernels of
// the device ones (*.hip). Both sides include this header, so a definition whose signature drifts from its caller's fails to
// compile (C linkage: a second signature under the same name is an error, not an overload). Argument blocks: abi_structs.hpp.
// A name ending in _docs is the DS2I_OP_TOPK_DOCS build of the launcher before it (the -DDS2I_DOCS_TU units of build.py: the same
// body over the (score, doc-id) heaps, defined under DS2I_KN(name), device_enum.hpp); same arguments, the docs fields of
// BatchArgs / MergeArgs set; ranked operators only, no counters.
#pragma once
#include <hip/hip_runtime.h>

#include "abi_structs.hpp"

extern "C" {
// ---- kernels.hip
// tmax_class: 0 -> TMAX 2, 1 -> TMAX 4, 2 -> TMAX 8, 3 -> TMAX 16 (LDS footprint per wave grows with TMAX), 4 -> more than 16 terms
// (state in global scratch); op: a ds2i_dev::OP_* value, | OP_REFERENCE_ORDER for the one-document-per-step traversal
hipError_t ds2i_launch_batch(int op, int tmax_class, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_batch_docs(int op, int tmax_class, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_merge(const ds2i_dev::MergeArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_merge_docs(const ds2i_dev::MergeArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_copy_seed(const ds2i_dev::CopySeedArgs& a, hipStream_t s);
hipError_t ds2i_launch_copy_seed_docs(const ds2i_dev::CopySeedDocsArgs& a, hipStream_t s);
uint32_t ds2i_meta_words(void); // dwords of enumerator state per list slot (M_WORDS)
hipError_t ds2i_launch_block_max_weights(const ds2i_dev::BmwArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_build_side_tables(const ds2i_dev::SideArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_list_top_bmw(const float* bmw, const ds2i_dev::QTerm* lists, uint32_t nlists, float* out, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_decode_list(const ds2i_dev::DecodeArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_decode_list_side(const ds2i_dev::DecodeArgs& a, unsigned grid, hipStream_t s);
// every block of every list against a staged collection; _side: block_optpfor through the side slots and the tail table
hipError_t ds2i_launch_verify_index(const ds2i_dev::VerifyArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_verify_index_side(const ds2i_dev::VerifyArgs& a, unsigned grid, hipStream_t s);
// the same walk over a block range, storing the postings in CSR form; _side: as above
hipError_t ds2i_launch_extract_index(const ds2i_dev::ExtractArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_extract_index_side(const ds2i_dev::ExtractArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_selftest(const uint32_t* in, uint32_t* out, unsigned blocks, hipStream_t s);
hipError_t ds2i_launch_selftest_bm25(const uint32_t* freqs, const float* norm_lens, float* out, uint32_t n, hipStream_t s);
hipError_t ds2i_launch_calib_read(const uint32_t* base, unsigned long long ndw, uint32_t* out, unsigned grid, hipStream_t s);

// ---- ranked_stream.hip (ranked_and; and / and_freq through the same pipeline), union_stream.hip (wand / maxscore / ranked_or).
// cap = list capacity of the launch (2, 4, 6, 8, 16); _bigk: 64 < k <= 1024, the units compiled with -DDS2I_RS_BIGK_TU / -DDS2I_US_BIGK_TU
hipError_t ds2i_launch_ranked_stream(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_ranked_stream_docs(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_ranked_stream_bigk(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_ranked_stream_bigk_docs(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_and_rstream(int cap, int with_freqs, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_union_stream(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_union_stream_docs(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_union_stream_bigk(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_union_stream_bigk_docs(int cap, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
// ---- ranked_stream_mixed.hip: nt = exact number of distinct terms of every query of the launch (2..4)
hipError_t ds2i_launch_ranked_stream_mixed(int nt, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_ranked_stream_mixed_docs(int nt, const ds2i_dev::BatchArgs& a, unsigned grid, hipStream_t s);

// ---- freq_stream.hip: longest = blocks of the longest list among the terms
hipError_t ds2i_launch_freq_stream(const ds2i_dev::FreqArgs& a, unsigned longest, unsigned nqterms, hipStream_t s);
hipError_t ds2i_launch_and_stream(const ds2i_dev::AndStreamArgs& a, int with_freqs, unsigned longest, unsigned nterms, hipStream_t s);

// ---- encode_kernels.hip, wand_kernels.hip
// mode: the codec_kind of the image (block_optpfor, block_varint, block_interpolative; block_mixed has a write pass only)
hipError_t ds2i_launch_encode(int mode, int write, const ds2i_dev::EncArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_hybrid_plan(const ds2i_dev::EncArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_wand_list_max(const uint32_t* docs, const uint32_t* freqs, const uint64_t* list_in, const uint32_t* blk_list,
                                     const uint32_t* list_blk0, uint32_t nblocks, const float* norm_lens, uint64_t num_docs,
                                     unsigned int* list_max, unsigned max_groups, hipStream_t s);
// ---- freq_encode_kernels.hip: the Elias-Fano layouts (opt, ef, single, uniform) over the same staging (EncArgs: freqs, list_in and the
// block tables). prefix_sums: cum[k] = sum of the freqs of k's list up to and including k (blk_base: nblocks words of scratch);
// write: the base sequences of one side (freqs_side: values from a.cum, else a.docs) ORed into the zero-filled a.out
hipError_t ds2i_launch_freq_prefix_sums(const ds2i_dev::EncArgs& st, uint64_t nlists, uint64_t* blk_base, uint64_t* cum, unsigned max_groups,
                                        hipStream_t s);
hipError_t ds2i_launch_freq_write(int freqs_side, const ds2i_dev::FreqEncArgs& a, unsigned max_groups, hipStream_t s);
// ---- partition_kernels.hip: the opt layout's partition end points (optimal_partition of host_pef.hpp) for a.nitems (list, side)
// items, one wavefront each. plan: the DP and the walk back (a.count, the end points in the item's scratch); gather: the end points
// to a.out_ends at a.out_offs
hipError_t ds2i_launch_partition_plan(const ds2i_dev::PartArgs& a, hipStream_t s);
hipError_t ds2i_launch_partition_gather(const ds2i_dev::PartArgs& a, hipStream_t s);
// ---- remap_kernels.hip: a staged collection renumbered through a doc-id map. grid: workgroups of 256 threads, which stride.
// map: a.docs through a.doc_map in place (a.flag: a doc-id outside the map); sort1 / sort2: the class 1 / class 2 lists from
// a.docs / a.freqs to a.out_docs / a.out_freqs; radix_pass: one pass of class 3 over the key bits from `shift` on, from the first
// buffer pair to the second or (from_second) back: the histogram, scan and scatter kernels, in that order, on s
hipError_t ds2i_launch_remap_map(const ds2i_dev::RemapArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_remap_sort1(const ds2i_dev::RemapArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_remap_sort2(const ds2i_dev::RemapArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_remap_radix_pass(const ds2i_dev::RemapArgs& a, int from_second, uint32_t shift, unsigned grid, hipStream_t s);
// ---- merge_kernels.hip: one source of a merge placed among the merged postings. grid: workgroups of 256 threads whose wavefronts
// stride over the windows of MERGE_WINDOW source postings
hipError_t ds2i_launch_merge_place(const ds2i_dev::MergePlaceArgs& a, unsigned grid, hipStream_t s);
// ---- split_kernels.hip: one shard of a split. grid: workgroups of SPLIT_THREADS threads whose wavefronts stride over the windows of
// SPLIT_WINDOW source postings (count, scatter) or over the source's list starts (offsets). count: a.win_count and a.flag; the host
// scans the counts into a.win_base; offsets: a.kept_before; scatter: the shard's postings with their local doc-ids
hipError_t ds2i_launch_split_count(const ds2i_dev::SplitArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_split_offsets(const ds2i_dev::SplitArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_split_scatter(const ds2i_dev::SplitArgs& a, unsigned grid, hipStream_t s);
// ---- invert_kernels.hip. grid: workgroups of SPLIT_THREADS threads. stage: every payload 1, a.flag for a token >= a.nterms (threads
// stride over the tokens); mark: the payload of every document's first token INVERT_DOC_START (threads stride over the documents);
// count / scatter: wavefronts stride over the windows of INVERT_WINDOW sorted tokens; offsets: over the ndocs + 1 document starts.
// transpose_count / transpose_scatter: wavefronts stride over the windows of INVERT_WINDOW entries
hipError_t ds2i_launch_invert_stage(const ds2i_dev::InvertArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_invert_mark(const ds2i_dev::InvertArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_invert_count(const ds2i_dev::InvertArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_invert_scatter(const ds2i_dev::InvertArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_invert_offsets(const ds2i_dev::InvertArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_transpose_count(const ds2i_dev::TransposeArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_transpose_scatter(const ds2i_dev::TransposeArgs& a, unsigned grid, hipStream_t s);
// ---- order_kernels.hip. grid: workgroups of SPLIT_THREADS threads. check, renumber, runs, degrees, gains: wavefronts stride over
// the windows of ORDER_WINDOW entries (check and renumber: threads over the entries); level, keys, presort_keys, swap, compose, finish:
// threads stride over the n positions. check: a.flag for a doc-id >= n; renumber: every entry through a.inv; level: half_of, side and
// members of a level's start; runs: back and run_len; degrees: deg_right; gains: gain; keys: (gain key, member) per slot;
// presort_keys: (member, member) per slot; swap: the exchanges of one iteration; compose: next_order and inv; finish: doc_map
hipError_t ds2i_launch_order_check(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_renumber(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_level(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_runs(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_degrees(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_gains(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_keys(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_presort_keys(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_swap(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_compose(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
hipError_t ds2i_launch_order_finish(const ds2i_dev::OrderArgs& a, unsigned grid, hipStream_t s);
// ---- shard_kernels.hip: grid workgroups of one wavefront stride over the a.nq queries; dynamic LDS = 24 * a.pow2 bytes
hipError_t ds2i_launch_merge_topk(const ds2i_dev::MergeTopkArgs& a, unsigned grid, hipStream_t s);
}
