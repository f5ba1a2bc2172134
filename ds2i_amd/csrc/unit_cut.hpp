// How a conjunctive query is cut into work units along the blocks of its shortest list (batch_plan.cpp, cut_units). Plain C++:
// nothing here knows about HIP, the index or the batch, so that a stand-alone program can check it (tests/unit_cut_check.cpp).
//
// Equal cut: `parts` = floor(cost / target), at least 1 and at most one per block; every part ceil(nb0 / parts) blocks, the last one
// what is left.
// Tapering cut (guided self-scheduling): the class order is costliest first and the hardware dispatches in that order, so the large
// parts of every split query start first, pay one prologue and one heap warm-up for many blocks and publish the query's floor while
// they run; the small parts start later, adopt that floor where they begin, and keep the kernel's tail as fine as the equal cut does.
// The first part is (1 - ratio) of the query, at most cap_mult equal parts and at least one; every next part is `ratio` times
// the previous one, never below the equal part. ratio = 1 or cap_mult = 1 IS the equal cut.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ds2i_cut {

// parts of the equal cut: one per `target` of cost, rounded down, at least one, at most one per block
inline uint32_t equal_parts(uint32_t nb0, double cost, double target) {
    nb0 = std::max(1u, nb0);
    if (!(cost > 0) || !(target > 0)) return 1;
    const double want = std::floor(cost / target);
    return (uint32_t)std::min<double>(std::max(1.0, want), (double)nb0);
}

// Cuts the blocks [0, nb0) into parts, given the part count of the equal cut: bounds = {0, b1, ..., nb0}, part j = [bounds[j], bounds[j + 1]).
// Sizes never grow from one part to the next, no part but the last is smaller than the equal part ceil(nb0 / parts), every part holds
// at least one block (so there are at most nb0 of them), and none holds more than cap_mult equal parts -- nor more than max_blocks
// blocks, if that is not 0 and the equal part itself keeps to it (a caller's bound on every unit: it chose `parts` for it, and the
// tapering must not undo it). Returns the number of parts.
inline uint32_t cut_blocks(uint32_t nb0, uint32_t parts, double ratio, double cap_mult, uint32_t max_blocks, std::vector<uint32_t>& bounds) {
    nb0 = std::max(1u, nb0);
    parts = std::min(std::max(1u, parts), nb0);
    ratio = ratio > 0 && ratio < 1 ? ratio : 1.0;
    cap_mult = cap_mult > 1 ? cap_mult : 1.0;
    const uint32_t per = (nb0 + parts - 1) / parts; // the equal part: the smallest a part may be
    const double first = std::min(std::ceil((double)nb0 * (1.0 - ratio)), std::min((double)nb0, cap_mult * (double)per));
    uint32_t size = std::max(per, (uint32_t)first);
    if (max_blocks) size = std::max(per, std::min(size, max_blocks));
    bounds.clear();
    bounds.push_back(0);
    for (uint32_t lo = 0; lo < nb0;) {
        lo += std::min(size, nb0 - lo);
        bounds.push_back(lo);
        size = std::max(per, (uint32_t)((double)size * ratio));
    }
    return (uint32_t)bounds.size() - 1;
}

// ... given the query's cost, the class's target cost of a unit and the cap on the largest part as a multiple of that target
inline uint32_t cut_query(uint32_t nb0, double cost, double target, double ratio, double cap_mult, std::vector<uint32_t>& bounds) {
    return cut_blocks(nb0, equal_parts(nb0, cost, target), ratio, cap_mult, 0, bounds);
}

// a part's cost: its share of the query's blocks
inline double part_cost(double cost, uint32_t nb0, uint32_t lo, uint32_t hi) { return cost * (double)(hi - lo) / (double)std::max(1u, nb0); }

} // namespace ds2i_cut
