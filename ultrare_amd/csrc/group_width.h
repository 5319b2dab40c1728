// group_width.h -- the widths a group of lanes may have, listed once.  The scoring family (score_dot.h, rec_score.h) groups
// LPR = d / 4 lanes round one (user, item) pair, the CSR walks (csr_lanes.h) G lanes round one row; both compile their kernels
// for every power of two up to the wavefront and pick one here.
#pragma once
#include <type_traits>

namespace ure {

// f(std::integral_constant<int, G>) for the group width G; false, and no call, for a width that is not listed.
template <typename F>
inline bool dispatch_group_width(int G, F &&f)
{
    switch (G) {
        case 1: f(std::integral_constant<int, 1>{}); return true;
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 4: f(std::integral_constant<int, 4>{}); return true;
        case 8: f(std::integral_constant<int, 8>{}); return true;
        case 16: f(std::integral_constant<int, 16>{}); return true;
        case 32: f(std::integral_constant<int, 32>{}); return true;
        case 64: f(std::integral_constant<int, 64>{}); return true;
    }
    return false;
}

}  // namespace ure
