// HIP kernels (gfx950, wave64) that INVERT documents into posting lists, and the primitive behind the inversion: the transposition of a
// sparse matrix in CSR form (capi_invert.cpp launches them; abi_structs.hpp: InvertArgs, TransposeArgs).
//
// From tokens to the canonical forward index. The tokens of every document have been sorted by the segmented sort of the remap
// (remap_kernels.hip) with a payload of 1 beside each. A RUN is a maximal stretch of equal tokens inside ONE document; its first token
// is its HEAD, its last its TAIL. Run r (counted over all tokens) becomes entry r: (term, freq = the run's length).
//   k_invert_stage    payload[i] = 1, grid-stride; a token at or past nterms raises a.flag (the host refuses: nothing later indexes a
//                     table by a token that was not checked)
//   k_invert_mark     after the sort every payload is 1 and says nothing: the payload of every nonempty document's first token becomes
//                     INVERT_DOC_START, so that head(i) = (i == 0 || payload[i] == INVERT_DOC_START || token[i] != token[i - 1]) needs
//                     no search for i's document. Two documents that end and begin with the same term do not fuse.
//   k_invert_count    per window of INVERT_WINDOW tokens, its heads: a ballot and a popcount per 64 tokens
//   (the host scans the window counts into u64: a.win_base, windows + 1 values)
//   k_invert_scatter  a wavefront walks a window with a running count that starts at the window's win_base. The run of token i is
//                     r = (heads at or before i) - 1, for every token of the run, wherever the run began: a run may span lanes, steps,
//                     windows and several whole windows. The head stores the term and adds -i to dst_freqs[r], the tail adds i + 1, in
//                     32-bit arithmetic: dst_freqs arrives zero-filled and ends as tail + 1 - head, the length (< 2^32, as a document's).
//                     Each word receives exactly two adds (one for a run of one token), so nothing contends and the sum has one value.
//   k_invert_offsets  per document start i = doc_first[d], the heads before i: win_base of i's window plus a ballot count over the
//                     window's tokens before i. A wavefront a start. An empty document gets its successor's value: an empty row.
//
// The transposition. Entries (column, value) lie row by row; the row of an entry is found as merge_kernels.hip finds a posting's list:
// once per window for its first and last entry by a binary search over all row starts, then per lane between those two.
//   k_transpose_count    count[column] += 1 (a vector atomic whose value is not used). A column at or past ncols, or one that does not
//                        exceed its left neighbour in the same row, raises a.flag and is not counted: nothing is indexed past count.
//   (the host scans the histogram into u64: a.col_first, ncols + 1 values, and zero-fills count again: the cursors)
//   k_transpose_scatter  entry i goes to col_first[c] + atomicAdd(&count[c], 1), a returning vector atomic add: (row, value). The order
//                        within a column is whatever the scheduling made it; the segmented sort puts every column in row order
//                        afterwards (row ids within a column are distinct, so the result is unique). All adds to one column's cursor
//                        serialise: a column present in every row costs one returning add per row on one word.
// No kernel waits for another workgroup. Every index comes from an offsets array, the scanned counts or a checked token; ragged last
// windows and steps are masked. Every loop's trip count is the same for all lanes of a wavefront, so every ballot sees the whole wavefront.
#include <hip/hip_runtime.h>

#include "launchers.hpp"

using namespace ds2i_dev;

namespace {

constexpr uint32_t THREADS = SPLIT_THREADS, WAVES = THREADS / 64;
static_assert(INVERT_WINDOW % 64 == 0, "a window is whole steps of a wavefront");

// token i (< a.n) begins a run
__device__ __forceinline__ bool is_head(const InvertArgs& a, uint64_t i) {
    return i == 0 || a.vals[i] == INVERT_DOC_START || a.keys[i] != a.keys[i - 1];
}
__device__ __forceinline__ bool head_below(const InvertArgs& a, uint64_t i, uint64_t end) { return i < end && is_head(a, i); }

__global__ void __launch_bounds__(THREADS) k_invert_stage(InvertArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < a.n; i += stride) {
        if (a.keys[i] >= a.nterms) atomicOr(a.flag, 1u);
        a.vals[i] = 1u;
    }
}

__global__ void __launch_bounds__(THREADS) k_invert_mark(InvertArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * THREADS;
    for (uint64_t d = (uint64_t)blockIdx.x * THREADS + threadIdx.x; d < a.ndocs; d += stride) {
        const uint64_t first = a.doc_first[d];
        if (first < a.doc_first[d + 1] && first < a.n) a.vals[first] = INVERT_DOC_START; // (the host checked the offsets: first < n)
    }
}

__global__ void __launch_bounds__(THREADS) k_invert_count(InvertArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwindows = (a.n + INVERT_WINDOW - 1) / INVERT_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * INVERT_WINDOW;
        const uint64_t w1 = w0 + INVERT_WINDOW < a.n ? w0 + INVERT_WINDOW : a.n;
        uint32_t count = 0;
        for (uint64_t i0 = w0; i0 < w1; i0 += 64) count += (uint32_t)__popcll(__ballot(head_below(a, i0 + lane, w1)));
        if (lane == 0) a.win_count[w] = count;
    }
}

__global__ void __launch_bounds__(THREADS) k_invert_offsets(InvertArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t d = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); d <= a.ndocs; d += nwaves) {
        const uint64_t i = a.doc_first[d] < a.n ? a.doc_first[d] : a.n; // (the host checked the offsets: i <= n)
        const uint64_t w = i / INVERT_WINDOW; // (i == n on a window boundary: w == windows, whose win_base is the total)
        uint32_t count = 0;
        for (uint64_t i0 = w * INVERT_WINDOW; i0 < i; i0 += 64) count += (uint32_t)__popcll(__ballot(head_below(a, i0 + lane, i)));
        if (lane == 0) a.heads_before[d] = a.win_base[w] + count;
    }
}

__global__ void __launch_bounds__(THREADS) k_invert_scatter(InvertArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t upto = lane == 63u ? ~0ull : (2ull << lane) - 1; // this lane and the ones below it
    const uint64_t nwindows = (a.n + INVERT_WINDOW - 1) / INVERT_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    const uint64_t total = a.win_base[nwindows];
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * INVERT_WINDOW;
        const uint64_t w1 = w0 + INVERT_WINDOW < a.n ? w0 + INVERT_WINDOW : a.n;
        uint64_t running = a.win_base[w];
        for (uint64_t i0 = w0; i0 < w1; i0 += 64) {
            const uint64_t i = i0 + lane;
            const bool valid = i < w1;
            const bool head = valid && is_head(a, i);
            const uint64_t heads = __ballot(head);
            const uint64_t at_or_before = running + (uint32_t)__popcll(heads & upto); // >= 1: token 0 is a head
            const bool tail = valid && (i + 1 == a.n || is_head(a, i + 1));
            if ((head || tail) && at_or_before >= 1 && at_or_before <= total) {
                const uint64_t r = at_or_before - 1;
                if (head) a.dst_terms[r] = a.keys[i];
                const uint32_t delta = (tail ? (uint32_t)(i + 1) : 0u) - (head ? (uint32_t)i : 0u);
                atomicAdd(&a.dst_freqs[r], delta);
            }
            running += (uint32_t)__popcll(heads);
        }
    }
}

// the largest t in [lo, hi] with first[t] <= i; the caller knows first[lo] <= i. Empty rows are skipped: the LAST row that starts at or
// before i is i's
__device__ __forceinline__ uint32_t row_of(const uint64_t* __restrict__ first, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <bool SCATTER>
__device__ __forceinline__ void transpose_walk(const TransposeArgs& a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwindows = (a.n + INVERT_WINDOW - 1) / INVERT_WINDOW;
    const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); w < nwindows; w += nwaves) {
        const uint64_t w0 = w * INVERT_WINDOW;
        const uint64_t w1 = w0 + INVERT_WINDOW < a.n ? w0 + INVERT_WINDOW : a.n;
        const uint32_t t_lo = row_of(a.row_first, 0, a.nrows - 1, w0); // (row_first[0] == 0 <= w0)
        const uint32_t t_hi = row_of(a.row_first, t_lo, a.nrows - 1, w1 - 1);
        for (uint64_t i = w0 + lane; i < w1; i += 64) {
            const uint32_t t = t_lo == t_hi ? t_lo : row_of(a.row_first, t_lo, t_hi, i);
            const uint32_t c = a.cols[i];
            if (!SCATTER) {
                if (c >= a.ncols || (i > a.row_first[t] && a.cols[i - 1] >= c)) atomicOr(a.flag, 1u);
                else atomicAdd(&a.count[c], 1u);
            } else if (c < a.ncols) {
                const uint64_t to = a.col_first[c] + atomicAdd(&a.count[c], 1u);
                if (to < a.col_first[c + 1]) { // (always, after a count that raised no flag)
                    a.out_rows[to] = t;
                    a.out_vals[to] = a.vals[i];
                }
            }
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_transpose_count(TransposeArgs a) { transpose_walk<false>(a); }
__global__ void __launch_bounds__(THREADS) k_transpose_scatter(TransposeArgs a) { transpose_walk<true>(a); }

} // namespace

extern "C" uint32_t ds2i_hip_invert_window(void) { return INVERT_WINDOW; }

#define DS2I_INVERT_LAUNCHER(name, kernel, Args, nonempty)                          \
    extern "C" hipError_t name(const Args& a, unsigned grid, hipStream_t s) {      \
        if (!(nonempty) || !grid) return hipSuccess;                                \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), 0, s, a);             \
        return hipGetLastError();                                                   \
    }
DS2I_INVERT_LAUNCHER(ds2i_launch_invert_stage, k_invert_stage, InvertArgs, a.n)
DS2I_INVERT_LAUNCHER(ds2i_launch_invert_mark, k_invert_mark, InvertArgs, a.n && a.ndocs)
DS2I_INVERT_LAUNCHER(ds2i_launch_invert_count, k_invert_count, InvertArgs, a.n)
DS2I_INVERT_LAUNCHER(ds2i_launch_invert_scatter, k_invert_scatter, InvertArgs, a.n)
DS2I_INVERT_LAUNCHER(ds2i_launch_invert_offsets, k_invert_offsets, InvertArgs, true)
DS2I_INVERT_LAUNCHER(ds2i_launch_transpose_count, k_transpose_count, TransposeArgs, a.n && a.nrows)
DS2I_INVERT_LAUNCHER(ds2i_launch_transpose_scatter, k_transpose_scatter, TransposeArgs, a.n && a.nrows)
#undef DS2I_INVERT_LAUNCHER
