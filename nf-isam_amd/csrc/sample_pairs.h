// sample_pairs.h — what the pairwise evaluators over the sample matrix share (sample_mmd.hip, sample_mmd_perm.hip, sample_ksd.hip, sample_svgd.hip;
// sample_modes.hip takes the host check of a block table, sample_knn.hip the tile's shape and tile_count, sample_density.hip tile_count): one level up from sample_common.h, which it includes, as
// factor_model.h is for the factor units.  Each unit still writes out its own walk over the pair tile -- coordinates, chunk
// loop, row lookup, block guard, wave combine: as shared helpers they cost registers or changed a kernel's listing
// (profiles/pair_tile_device_code.txt).
#pragma once
#include <stdint.h>

#include "sample_common.h"

namespace sample_pairs {

using namespace sample_common;

constexpr int TILE = 64;          // pairs tile: 64 i (one per lane) x 64 j (16 per wave-lane, 4 waves)
constexpr int JPL = 16;           // j per lane
constexpr int CH = 16;            // columns per staged chunk
static_assert(TILE == 64, "one i per lane of a wave");
static_assert(4 * JPL == TILE, "the four waves share the tile's j");
static_assert(CH % 4 == 0, "wave w stages columns w, w + 4, ...");

// the number of 64-wide tiles over n points, if a grid's second dimension can hold it
inline bool tile_count(int n, int* T) {
    if (n < 1) return false;
    const long long t = ((long long)n + TILE - 1) / TILE;
    if (t > 65535) return false;
    *T = (int)t;
    return true;
}

// sign(d) wrap(|d|): d_ji = -d_ij to the bit, which H's symmetry (KSD) and the swap promise of the SVGD direction rest on.
// sample_mmd.hip wraps with wrap_pi(diff) instead, the form its sums were first recorded with, and keeps those bits.
__device__ __forceinline__ double signed_wrap(double d) {
    const double m = wrap_pi_near(fabs(d));
    return (d < 0.0) ? -m : m;
}

// the HOST copy of a block table, read before the launch: every block has 1 <= d <= max_d and a finite positive bandwidth
static_assert(sizeof(nfisam_mmd_block) == 16, "nfisam_mmd_block is 16 bytes");
inline bool check_block_table(const nfisam_mmd_block* blocks, int n_blocks, int max_d = 2147483647) {
    for (int b = 0; b < n_blocks; ++b) {
        const double v = blocks[b].inv_two_sigma2;
        if (blocks[b].d < 1 || blocks[b].d > max_d || !(v > 0.0) || !isfinite(v)) return false;
    }
    return true;
}

}  // namespace sample_pairs
