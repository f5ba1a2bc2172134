// Launcher-side dispatch: each helper turns one run-time value into a compile-time constant and calls a generic callable with it
// (f(std::integral_constant) -> hipError_t), so that a launcher states its kernel's template arguments once, and which
// instantiation of a kernel family a launch takes is decided in one place (specialised / instrumented below).
// Host code only, for the *.hip units.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_codecs.hpp" // CODEC_*
#include "device_pef.hpp"    // CODEC_PEF

namespace ds2i_launch {
using namespace ds2i_dev;

#ifdef DS2I_DOCS_TU
constexpr bool DOCS_TU = true; // a *_docs unit of build.py (device_enum.hpp, DS2I_KN)
#else
constexpr bool DOCS_TU = false;
#endif

template <int V> using Int = std::integral_constant<int, V>;

// f(Int<V>) for the V among Vs that equals v; a value outside the set is refused
template <int... Vs, class F>
hipError_t pick(int v, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs && ((e = f(Int<Vs>{})), true)) || ...);
    return e;
}
template <class F> hipError_t with_cap(int cap, F&& f) { return pick<2, 4, 6, 8, 16>(cap, f); }   // list capacity of a stream launch
template <class F> hipError_t with_lists(int nt, F&& f) { return pick<2, 3, 4>(nt, f); }          // exact list count (k_ranked_stream_mixed)
template <class F> hipError_t with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// scores per lane of the top-k heap: k <= 64 -> 1, k <= 256 -> 4, k <= 1024 -> 16; the _bigk units hold the last two only
template <class F> hipError_t with_big_heap(uint32_t k, F&& f) { return k <= 256 ? f(Int<4>{}) : f(Int<16>{}); }
template <class F> hipError_t with_heap(uint32_t k, F&& f) { return k <= 64 ? f(Int<1>{}) : with_big_heap(k, f); }
// The codec a class kernel may be specialised for: block_optpfor counts only with the upload-time side tables (an index uploaded
// without them decodes through the runtime-codec instantiation, -1, like block_varint / block_interpolative / block_qmx)
template <class F>
hipError_t with_codec(const BatchArgs& a, F&& f) {
    if (a.codec == CODEC_OPTPFOR && a.xslots != nullptr && a.tails != nullptr) return f(Int<CODEC_OPTPFOR>{});
    if (a.codec == CODEC_PEF) return f(Int<CODEC_PEF>{});
    if (a.codec == CODEC_MIXED) return f(Int<CODEC_MIXED>{});
    return f(Int<-1>{});
}

template <class A>
hipError_t launch(void (*kernel)(A), dim3 grid, dim3 block, size_t dyn_lds, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, grid, block, dyn_lds, s, a);
    return hipGetLastError();
}

// ---- which instantiations exist. The set is irregular on purpose (every instantiation costs build time and code size; the
// uninstrumented ones exist where a benchmark configuration runs them) and this is the one place that states it.
enum Family { K_CONJUNCTIVE, K_DISJUNCTIVE, K_UNION_TOPK, K_UNION, K_STREAM /* k_ranked_stream[_mixed], k_union_stream: one codec each */ };

// CODEC_T of the instantiation that serves `codec` (a with_codec value): the family's own specialisation, else runtime dispatch
constexpr int specialised(Family f, int codec) {
    const bool own = codec == CODEC_OPTPFOR || (codec == CODEC_PEF && f != K_UNION) || (codec == CODEC_MIXED && f != K_UNION && f != K_UNION_TOPK);
    return own ? codec : -1;
}
// STATS of the instantiation a launch takes (codec: a specialised() value). A docs unit holds uninstrumented kernels only (a docs
// batch passes no counters). Elsewhere the instantiation with counters always exists, and one without them for block_optpfor, and
// for the freq_index family in k_conjunctive: a run without counters on any other codec (k_ranked_stream_mixed among them)
// shares the instrumented instantiation.
constexpr bool instrumented(Family f, int codec, bool counters) {
    if (DOCS_TU) return false;
    const bool lean_exists = codec == CODEC_OPTPFOR || (codec == CODEC_PEF && f == K_CONJUNCTIVE);
    return counters || !lean_exists;
}

} // namespace ds2i_launch
