// HIP class kernels (gfx950 / CDNA4, wave64) of the ds2i batched query path: everything the stream kernels (ranked_stream.hip,
// union_stream.hip, freq_stream.hip) do not answer, the reference-order traversals, and the upload-time passes.
// One wavefront per WORK UNIT (a piece of a query: a block range of its shortest list, or a doc-id range), one unit per single-wave
// workgroup; every memory operation is wave-cooperative, control flow is wave-uniform. No MFMA (integer work).
// The kernels live in one include file per operator family; this file holds their launchers (declared in launchers.hpp, called
// from capi*.cpp; which instantiation a launch takes: dispatch.hpp):
//   kernels_common.inc        per-wave LDS layout, enumerator construction, top-k stores
//   kernels_conjunctive.inc   k_conjunctive  and_query / ranked_and_query (queries.hpp:35-86, 322-401), block-synchronous; k_merge
//   kernels_daat.inc          k_daat / k_daat_long  every operator in the reference's one-document-per-step order
//                             (DS2I_OP_REFERENCE_ORDER; > 16 terms; k > 64)
//   kernels_disjunctive.inc   k_disjunctive, k_union_topk  wand / maxscore / ranked_or (queries.hpp:200-319, 404-476, 478-591) without
//                             side slots / range tables; k_union  or / or_freq (queries.hpp:88-131) as a stream
//   kernels_upload.inc        view_batch_args (the decoders' BatchArgs of an IndexView), k_decode_list[_side], the whole-index walk (walk_index[_side]
//                             over WalkArgs) under k_verify_index[_side] and k_extract_index[_side], k_block_max_weights, k_build_side_tables,
//                             k_list_top_bmw, self-tests
// Compiled once per list-count class (-DDS2I_TU_TMAX=2|4|8|16: launch_t<TMAX> and the kernels it instantiates; =0: launch_long, the
// class of more than 16 terms) and once without the macro (the entry points and everything else): six translation units that
// build.py compiles in parallel -- the kernel templates are by far the slowest part of the build. The five class units are
// compiled once more with -DDS2I_DOCS_TU (DS2I_OP_TOPK_DOCS): the same launcher bodies under the names DS2I_KN gives them, over the
// ranked operators' kernels with the (score, doc-id) heaps (device_enum.hpp), uninstrumented; the docs entry points live in
// the =0 unit. k_daat / k_daat_long have no STATS parameter and count into nothing when a.stats is null.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_enum.hpp"
#include "device_score.hpp"
#include "dispatch.hpp"
#include "launchers.hpp"

using namespace ds2i_dev;

namespace {
#include "kernels_common.inc"
#include "kernels_conjunctive.inc"
#include "kernels_daat.inc"
#include "kernels_disjunctive.inc"
#include "kernels_upload.inc"

} // namespace

// ------------------------------------------------------------------ launchers
namespace ds2i_launch {

// the operators a unit builds kernels for: all eight; a docs unit the ranked four
template <class F>
hipError_t with_op(int op, F&& f) {
    if constexpr (DOCS_TU) return pick<OP_RANKED_AND, OP_WAND, OP_MAXSCORE, OP_RANKED_OR>(op, f);
    else return pick<OP_AND, OP_AND_FREQ, OP_OR, OP_OR_FREQ, OP_RANKED_AND, OP_WAND, OP_MAXSCORE, OP_RANKED_OR>(op, f);
}

template <int TMAX>
hipError_t DS2I_KN(launch_t)(int op, const BatchArgs& a, unsigned grid, hipStream_t s);
hipError_t DS2I_KN(launch_long)(int op, const BatchArgs& a, unsigned grid, hipStream_t s);

#if defined(DS2I_TU_TMAX) && DS2I_TU_TMAX > 0
template <int TMAX>
hipError_t DS2I_KN(launch_t)(int op, const BatchArgs& a, unsigned grid, hipStream_t s) {
    const dim3 g(grid), b(64);
    return with_op(op & 0xFF, [&](auto o) {
        constexpr int OP = decltype(o)::value;
        // reference-order (one document / one candidate per step) traversal of the operator: op | OP_REFERENCE_ORDER
        if (op & OP_REFERENCE_ORDER) return launch(DS2I_KN(k_daat)<OP, TMAX>, g, b, 0, s, a);
        // the conjunctive kernels are specialised for block_optpfor (the benchmark codec), the freq_index family and
        // block_mixed (configs[4]; its three block types stay a run-time switch, QMX drops out)
        if constexpr (OP == OP_AND || OP == OP_AND_FREQ || OP == OP_RANKED_AND) {
            return with_codec(a, [&](auto c) { return with_bool(a.stats != nullptr, [&](auto counters) {
                constexpr int C = specialised(K_CONJUNCTIVE, decltype(c)::value);
                return launch(DS2I_KN(k_conjunctive)<OP == OP_RANKED_AND, OP != OP_AND, TMAX, C, instrumented(K_CONJUNCTIVE, C, decltype(counters)::value)>, g, b, 0, s, a);
            }); });
        } else if constexpr (OP == OP_OR || OP == OP_OR_FREQ) {
            return hipErrorInvalidValue; // or / or_freq run k_union for every list count (ds2i_launch_batch below)
        } else { // wand / maxscore / ranked_or (identical results by definition)
            return with_codec(a, [&](auto c) { return with_bool(a.stats != nullptr, [&](auto counters) {
                if (a.vq_info) { // the streaming form (units = (query, driving list, block range)); needs the range tables
                    constexpr int C = specialised(K_UNION_TOPK, decltype(c)::value);
                    return launch(DS2I_KN(k_union_topk)<TMAX, C, instrumented(K_UNION_TOPK, C, decltype(counters)::value)>, g, b, 0, s, a);
                }
                // the block-synchronous disjunctive kernel; dynamic LDS: docs + freqs of dyn_lists list slots
                constexpr int C = specialised(K_DISJUNCTIVE, decltype(c)::value);
                return launch(DS2I_KN(k_disjunctive)<TMAX, C, instrumented(K_DISJUNCTIVE, C, decltype(counters)::value)>, g, b, 1024u * (size_t)a.dyn_lists, s, a);
            }); });
        }
    });
}
template hipError_t DS2I_KN(launch_t)<DS2I_TU_TMAX>(int, const BatchArgs&, unsigned, hipStream_t);
#elif defined(DS2I_TU_TMAX)
// the "long" class: k_daat_long, every operator in reference order; k > 64: sixteen scores per lane (k <= 1024), ranked operators only
hipError_t DS2I_KN(launch_long)(int op, const BatchArgs& a, unsigned grid, hipStream_t s) {
    const dim3 g(grid), b(64);
    return with_op(op & 0xFF, [&](auto o) {
        constexpr int OP = decltype(o)::value;
        if (a.k <= 64) return launch(DS2I_KN(k_daat_long)<OP>, g, b, 0, s, a);
        if constexpr (OP >= OP_RANKED_AND) return launch(DS2I_KN(k_daat_long)<OP, RTopKBig<16>>, g, b, 0, s, a);
        else return hipErrorInvalidValue;
    });
}
#endif

} // namespace ds2i_launch

// The entry points: in the unit compiled without -DDS2I_TU_TMAX; the docs build has no such unit and keeps them in its long unit
#if defined(DS2I_DOCS_TU) ? DS2I_TU_TMAX == 0 : !defined(DS2I_TU_TMAX)
using namespace ds2i_launch;
extern "C" {

hipError_t DS2I_KN(ds2i_launch_batch)(int op, int tmax_class, const BatchArgs& a, unsigned grid, hipStream_t s) {
#ifndef DS2I_DOCS_TU
    if ((op == OP_OR || op == OP_OR_FREQ) && a.dyn_lists == 0xFFFFFFFFu) // or_query as a stream: one kernel for every list count
        return with_codec(a, [&](auto c) { return with_bool(op == OP_OR_FREQ, [&](auto f) { return with_bool(a.stats != nullptr, [&](auto counters) {
            constexpr int C = specialised(K_UNION, decltype(c)::value);
            return launch(k_union<decltype(f)::value, C, instrumented(K_UNION, C, decltype(counters)::value)>, dim3(grid), dim3(64), 0, s, a);
        }); }); });
#endif
    switch (tmax_class) {
    case 0: return DS2I_KN(launch_t)<2>(op, a, grid, s);
    case 1: return DS2I_KN(launch_t)<4>(op, a, grid, s);
    case 2: return DS2I_KN(launch_t)<8>(op, a, grid, s);
    case 3: return DS2I_KN(launch_t)<16>(op, a, grid, s);
    default: return DS2I_KN(launch_long)(op, a, grid, s);
    }
}

// the unranked merge keeps one kernel for every k; a docs batch has none
hipError_t DS2I_KN(ds2i_launch_merge)(const MergeArgs& a, unsigned grid, hipStream_t s) {
    if (DOCS_TU && !a.ranked) return hipErrorInvalidValue;
    return with_heap(a.ranked ? a.k : 0u, [&](auto nk) {
        constexpr int NK = decltype(nk)::value;
        if constexpr (NK == 1) return launch(DS2I_KN(k_merge), dim3(grid), dim3(64), 0, s, a);
        else return launch(DS2I_KN(k_merge_big)<NK>, dim3(grid), dim3(64), 0, s, a);
    });
}

#ifdef DS2I_DOCS_TU
hipError_t ds2i_launch_copy_seed_docs(const CopySeedDocsArgs& a, hipStream_t s) {
    return launch(k_copy_seed_docs, dim3(a.s.n < 1024 ? a.s.n : 1024), dim3(64), 0, s, a);
}
#else
hipError_t ds2i_launch_copy_seed(const CopySeedArgs& a, hipStream_t s) {
    return launch(k_copy_seed, dim3(a.n < 1024 ? a.n : 1024), dim3(64), 0, s, a);
}

uint32_t ds2i_meta_words(void) { return (uint32_t)M_WORDS; }

hipError_t ds2i_launch_block_max_weights(const BmwArgs& a, unsigned grid, hipStream_t s) { return launch(k_block_max_weights, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_build_side_tables(const SideArgs& a, unsigned grid, hipStream_t s) { return launch(k_build_side_tables, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_decode_list_side(const DecodeArgs& a, unsigned grid, hipStream_t s) { return launch(k_decode_list_side, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_decode_list(const DecodeArgs& a, unsigned grid, hipStream_t s) { return launch(k_decode_list, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_verify_index(const VerifyArgs& a, unsigned grid, hipStream_t s) { return launch(k_verify_index, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_verify_index_side(const VerifyArgs& a, unsigned grid, hipStream_t s) { return launch(k_verify_index_side, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_extract_index(const ExtractArgs& a, unsigned grid, hipStream_t s) { return launch(k_extract_index, dim3(grid), dim3(64), 0, s, a); }
hipError_t ds2i_launch_extract_index_side(const ExtractArgs& a, unsigned grid, hipStream_t s) { return launch(k_extract_index_side, dim3(grid), dim3(64), 0, s, a); }

hipError_t ds2i_launch_list_top_bmw(const float* bmw, const QTerm* lists, uint32_t nlists, float* out, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL(k_list_top_bmw, dim3(grid), dim3(64), 0, s, bmw, lists, nlists, out);
    return hipGetLastError();
}

hipError_t ds2i_launch_selftest(const uint32_t* in, uint32_t* out, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest, dim3(blocks), dim3(64), 0, s, in, out);
    return hipGetLastError();
}

hipError_t ds2i_launch_selftest_bm25(const uint32_t* freqs, const float* norm_lens, float* out, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest_bm25, dim3((n + 63) / 64), dim3(64), 0, s, freqs, norm_lens, out, n);
    return hipGetLastError();
}

hipError_t ds2i_launch_calib_read(const uint32_t* base, unsigned long long ndw, uint32_t* out, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL(k_calib_read, dim3(grid), dim3(64), 0, s, base, ndw, out);
    return hipGetLastError();
}
#endif
}
#endif
