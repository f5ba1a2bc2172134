// Stand-alone check of ds2i_amd/csrc/unit_cut.hpp (no HIP, its own main): the properties cut_units relies on, swept over block counts,
// costs, ratios and caps. Built with -fsanitize=address,undefined and run by tests/test_unit_cut_cpu.py. Prints "unit_cut: ..." and
// returns 0 when every case holds; the first failure is printed and the exit status is 1.
#include <cstdio>
#include <cstdlib>

#include "../ds2i_amd/csrc/unit_cut.hpp"

static unsigned long long cases = 0;

[[noreturn]] static void fail(const char* what, uint32_t nb0, double cost, double target, double ratio, double mult) {
    std::printf("unit_cut FAILED: %s (nb0 %u cost %g target %g ratio %g cap multiple %g)\n", what, nb0, cost, target, ratio, mult);
    std::exit(1);
}

// today's equal cut, written out as cut_units had it
static void equal_cut_reference(uint32_t nb0, double cost, double target, std::vector<uint32_t>& bounds) {
    uint32_t parts = 1;
    if (nb0 > 1) parts = (uint32_t)std::min<double>(std::max(1.0, std::floor(cost / target)), nb0);
    nb0 = std::max(1u, nb0);
    const uint32_t per = (nb0 + parts - 1) / parts;
    parts = (nb0 + per - 1) / per;
    bounds.clear();
    for (uint32_t j = 0; j < parts; ++j) bounds.push_back(j * per);
    bounds.push_back(nb0);
}

static void check(uint32_t nb0, double cost, double target, double ratio, double mult) {
    ++cases;
    std::vector<uint32_t> b, again, eq;
    const uint32_t parts = ds2i_cut::cut_query(nb0, cost, target, ratio, mult, b);
    if (parts < 1 || parts > nb0 || b.size() != (size_t)parts + 1) fail("part count outside [1, nb0]", nb0, cost, target, ratio, mult);
    if (b.front() != 0 || b.back() != nb0) fail("parts do not cover [0, nb0)", nb0, cost, target, ratio, mult);
    const uint32_t p_eq = ds2i_cut::equal_parts(nb0, cost, target);
    if (p_eq < 1 || p_eq > nb0) fail("equal part count outside [1, nb0]", nb0, cost, target, ratio, mult);
    const uint32_t per = (nb0 + p_eq - 1) / p_eq;
    if (parts > (nb0 + per - 1) / per) fail("more parts than the equal cut", nb0, cost, target, ratio, mult);
    double cost_sum = 0;
    for (uint32_t j = 0; j < parts; ++j) {
        if (b[j + 1] <= b[j]) fail("empty or overlapping part", nb0, cost, target, ratio, mult);
        const uint32_t size = b[j + 1] - b[j];
        if (j && size > b[j] - b[j - 1]) fail("a part is larger than the one before it", nb0, cost, target, ratio, mult);
        if (j + 1 < parts && size < per) fail("a part other than the last is below the equal part", nb0, cost, target, ratio, mult);
        if ((double)size > std::max(1.0, mult) * (double)per) fail("a part is above the cap", nb0, cost, target, ratio, mult);
        cost_sum += ds2i_cut::part_cost(cost, nb0, b[j], b[j + 1]);
    }
    if (std::fabs(cost_sum - cost) > 1e-9 * std::max(1.0, cost)) fail("part costs do not add up to the query's", nb0, cost, target, ratio, mult);
    ds2i_cut::cut_query(nb0, cost, target, ratio, mult, again);
    if (again != b) fail("two calls disagree", nb0, cost, target, ratio, mult);
    if (ratio == 1.0 || mult == 1.0) {
        equal_cut_reference(nb0, cost, target, eq);
        if (eq != b) fail("ratio 1 / cap = target is not the equal cut", nb0, cost, target, ratio, mult);
    }
}

int main() {
    const uint32_t nbs[] = {1, 2, 63, 64, 65, 1000, 1u << 25};
    const double targets[] = {48.0, 256.0, 1777.25};
    const double rel_costs[] = {0.0, 0.5, 0.999, 1.0, 1.5, 2.0, 3.0, 3.999, 4.0, 7.0, 8.0, 9.5, 16.0, 31.0, 64.0, 100.0, 1000.0, 65536.0, 1.0e6, 33554432.0, 1.0e9};
    const double ratios[] = {1.0, 0.5, 2.0 / 3.0, 0.25, 0.9};
    const double mults[] = {1.0, 2.0, 4.0, 8.0, 3.5, 1.0e9};
    for (uint32_t nb0 : nbs)
        for (double target : targets)
            for (double rc : rel_costs)
                for (double ratio : ratios)
                    for (double mult : mults) {
                        // (up to 33 M parts each: one target and two shapes suffice)
                        if (nb0 == (1u << 25) && rc > 1000.0 && !(target == 256.0 && ((ratio == 1.0 && mult == 1.0) || (ratio == 0.5 && mult == 8.0)))) continue;
                        check(nb0, rc * target, target, ratio, mult);
                    }
    // every block count up to a few tiles, the grid cut_units chooses from
    for (uint32_t nb0 = 1; nb0 <= 300; ++nb0)
        for (double rc : {1.0, 2.5, 4.0, 6.0, 11.0, 40.0, 299.0, 300.0, 301.0})
            for (double ratio : {1.0, 0.5, 2.0 / 3.0})
                for (double mult : {1.0, 2.0, 4.0, 8.0}) check(nb0, rc * 256.0, 256.0, ratio, mult);
    // a tapering cut of a long query is unequal and has fewer parts than the equal cut
    std::vector<uint32_t> b;
    const uint32_t parts = ds2i_cut::cut_query(1000, 20.0 * 256.0, 256.0, 0.5, 8.0, b);
    if (!(parts >= 4 && parts < 20 && b[1] - b[0] == 400 && b[2] - b[1] == 200 && b[3] - b[2] == 100 && b[4] - b[3] == 50 && b[parts] - b[parts - 1] == 50))
        fail("the tapering cut of 1000 blocks in 20 targets is not 400, 200, 100, 50 ...", 1000, 20.0 * 256.0, 256.0, 0.5, 8.0);
    // out-of-range arguments fall back to the equal cut instead of misbehaving
    for (double ratio : {0.0, -1.0, 2.0, std::nan("")})
        for (double mult : {0.0, -3.0, 0.5, std::nan("")}) {
            std::vector<uint32_t> eq;
            ds2i_cut::cut_query(1000, 5000.0, 256.0, ratio, mult, b);
            equal_cut_reference(1000, 5000.0, 256.0, eq);
            if (b != eq) fail("out-of-range ratio / cap is not the equal cut", 1000, 5000.0, 256.0, ratio, mult);
        }
    // a caller's bound on the blocks of a unit (DS2I_UNIT_CAP): parts chosen for it, and no part of the tapering cut exceeds it
    for (uint32_t nb0 : {1u, 7u, 8u, 9u, 63u, 64u, 65u, 100u, 141u, 512u, 1000u, 4097u})
        for (uint32_t bound : {1u, 4u, 8u, 96u})
            for (double rc : {0.0, 1.0, 3.0, 20.0, 500.0})
                for (double ratio : {1.0, 0.5, 2.0 / 3.0})
                    for (double mult : {1.0, 2.0, 4.0, 8.0}) {
                        ++cases;
                        const uint32_t want = std::max(ds2i_cut::equal_parts(nb0, rc * 256.0, 256.0), (nb0 + bound - 1) / bound);
                        const uint32_t n = ds2i_cut::cut_blocks(nb0, want, ratio, mult, bound, b);
                        if (n < 1 || n > nb0 || b.size() != (size_t)n + 1 || b.front() != 0 || b.back() != nb0) fail("bounded cut does not cover [0, nb0)", nb0, rc * 256.0, 256.0, ratio, mult);
                        for (uint32_t j = 0; j < n; ++j) {
                            if (b[j + 1] <= b[j] || b[j + 1] - b[j] > bound) fail("a part exceeds the caller's block bound", nb0, rc * 256.0, 256.0, ratio, mult);
                            if (j && b[j + 1] - b[j] > b[j] - b[j - 1]) fail("bounded cut: a part is larger than the one before it", nb0, rc * 256.0, 256.0, ratio, mult);
                        }
                    }
    std::printf("unit_cut: %llu cases hold\n", cases);
    return 0;
}
