// Stand-alone check (its own main, no HIP) of RmwLevels::bitmap_first (ds2i_amd/csrc/abi_structs.hpp), the rule by which
// k_ranked_stream fetches list 1's bitmap byte ahead instead of its hint byte: over a sweep of (n, num_docs, shift) it must hold
// exactly where the list has a bitmap and a 128-byte line of the bitmap (1024 doc-ids) covers no fewer doc-ids than a 128-byte line
// of the list's level-1 table (128 entries of 1 << shift doc-ids); and where it holds, the bitmap byte of every doc-id lies inside
// the bitmap (bitmap_bytes), which starts at the end of the levels (bytes()).
#define __host__
#define __device__
#include <cstdio>

#include "../ds2i_amd/csrc/abi_structs.hpp"

int main() {
    using ds2i_dev::RmwLevels;
    unsigned long long checked = 0, held = 0;
    const uint32_t docs[] = {1u, 63u, 64u, 65u, 1000u, 16384u, 16385u, 1000003u, 25000000u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t nd : docs) {
        for (uint32_t shift = 0; shift < 32; ++shift) {
            const uint32_t edge = (uint32_t)(((uint64_t)nd + 63u) / 64u); // the fewest postings with a bitmap
            const uint32_t ns[] = {1u, edge ? edge - 1u : 0u, edge, edge + 1u, nd / 2u + 1u, nd};
            for (uint32_t n : ns) {
                if (n == 0 || n > nd) continue;
                const bool has = (uint64_t)n * 64u >= (uint64_t)nd;
                const bool dense_enough = (128ull << shift) <= 1024ull;
                const bool got = RmwLevels::bitmap_first(n, nd, shift);
                ++checked;
                if (has != RmwLevels::has_bitmap(n, nd) || got != (has && dense_enough)) {
                    std::printf("FAIL n=%u num_docs=%u shift=%u: %d\n", n, nd, shift, (int)got);
                    return 1;
                }
                if (got) {
                    ++held;
                    const RmwLevels g(nd, shift);
                    if (g.bytes() % 64u != 0 || (uint64_t)((nd - 1u) >> 3) >= RmwLevels::bitmap_bytes(nd) - 64u) {
                        std::printf("FAIL geometry num_docs=%u shift=%u\n", nd, shift);
                        return 1;
                    }
                }
            }
        }
    }
    std::printf("bitmap_first: %llu cases checked, %llu hold\n", checked, held);
    return held > 0 && held < checked ? 0 : 1;
}
