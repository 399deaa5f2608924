// sample_common.h — what the float64 evaluators over the column-major sample matrix share (factor_density.hip,
// factor_score.hip, sample_mmd.hip, sample_mmd_perm.hip, sample_ksd.hip, sample_svgd.hip, sample_summary.hip, sample_modes.hip, sample_mcmc.hip, sample_chains.hip, sample_knn.hip, sample_density.hip, sample_trajectory.hip, sample_transport.hip): the angle wrap, the wave
// reductions, the launch epilogue.  A new evaluator over that matrix starts from this header -- one of the FACTORS from
// factor_model.h, which includes it and holds the factor model the two factor units share, one over PAIRS of points from
// sample_pairs.h, which includes it and holds what the MMD, KSD and SVGD units share; it does NOT include nsf_host.h
// (the flow kernels' headers and `using namespace nsf`, whose float wave_sum / wrap_pi are other functions).
//
// THE MATRIX AND THE NUMERICS.  The points are the COLUMN-major float32 device matrix [rows][n] that the tree walk writes (St):
// row r holds coordinate r of all n points, so a lane per point reads coalesced.  float32 points in; every difference,
// product, transcendental and sum is float64, and results leave as float64 -- the value of the float64 formula at the float32
// point.  (Coordinates reach 100 m with spreads of centimetres, and the joint density reaches 1e11.)
//
// THE REDUCTION ORDER.  Every unit promises that two calls give the same bits and that a block's results do not depend on
// where it stands in a table.  The promise rests on every float64 sum being taken in one fixed order, by these helpers:
//   - a thread adds its own terms in ascending index order;
//   - wave_sum: a fixed shuffle tree over the 64 lanes, offsets 32, 16, ..., 1 (lane 0 holds the sum);
//   - waves_in_order: the four waves of a 256-thread group, ((p[0] + p[1]) + p[2]) + p[3].
// No float atomics anywhere.  Change an order here and every unit's bits change together; change it in one unit's own copy
// and the units disagree -- which is why there are no copies.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/nfisam_hip.h"

extern thread_local int nfisam_g_last_hip_error;      // defined in the common unit (nsf_kernels.hip)

namespace sample_common {

constexpr double TWO_PI = 6.283185307179586476925286766559;
constexpr double PI = 3.141592653589793238462643383279;

// (t + pi) mod 2 pi - pi with the sign of Python's `%` (utils/Functions.py:20-21 theta_to_pipi): [-pi, pi).  The plain form:
// for an argument that may lie anywhere (a residual of headings, a key about a centre), and wherever the wrap is rare.
__device__ __forceinline__ double wrap_pi(double t) {
    double m = fmod(t + PI, TWO_PI);
    if (m < 0.0) m += TWO_PI;
    return m - PI;
}

// The same value, bit for bit: where 0 <= t + pi < 2 pi the remainder is t + pi itself and fmod is not called.  For an inner
// loop whose arguments are differences of wrapped angles and mostly in range already (the mean-shift ascent).
__device__ __forceinline__ double wrap_pi_near(double t) {
    double m = t + PI;
    if (!(m >= 0.0 && m < TWO_PI)) {
        m = fmod(m, TWO_PI);
        if (m < 0.0) m += TWO_PI;
    }
    return m - PI;
}

__device__ __forceinline__ double wave_sum(double v) {           // a fixed tree: the same order in every wave of every call
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                      // (lane 0 holds the sum)
}

__device__ __forceinline__ double wave_total(double v) {         // the same tree, the sum in every lane
    return __shfl(wave_sum(v), 0, 64);
}

// the four waves' partial sums (lane 0's wave_sum, parked in LDS), in wave order
__device__ __forceinline__ double waves_in_order(const double* p) { return ((p[0] + p[1]) + p[2]) + p[3]; }

// the epilogue of an entry point: NFISAM_OK, or NFISAM_ERR_LAUNCH with the HIP error kept for nfisam_last_hip_error()
inline int launch_status(hipError_t e) {
    if (e == hipSuccess) return NFISAM_OK;
    nfisam_g_last_hip_error = (int)e;
    return NFISAM_ERR_LAUNCH;
}

}  // namespace sample_common
