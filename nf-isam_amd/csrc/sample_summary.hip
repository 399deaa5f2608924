// sample_summary.hip — what a sample set says: means, resultant lengths, covariances and quantiles of many column blocks.
//
// The reference summarises a posterior draw on the host (src/utils/Statistics.py:142-214: `sample_mean` with scipy's circmean
// for headings, `rmse`, `translation_distance`, `geodesic_distance`); its run scripts copy the whole [n, total_dim] matrix
// out and loop over the variables in numpy after every update.  Here the matrix is summarised where the tree walk wrote it:
// Xt is the COLUMN-major float32 device matrix [x_rows][n] (the walk's St, the layout of sample_common.h); an entry e names
// a row cols[e] of Xt (one coordinate of one variable) and a block is a run of entries.
//
// Numerics: float32 points in; every difference, product, transcendental and sum is float64 (the contract of
// sample_common.h).  TWO PASSES: the means first, then residuals about the float64 mean -- never
// sum x^2 - (sum x)^2, which cancels at coordinates of 100 m and spreads of centimetres.  Both means are taken about the
// column's first point: x_0 + sum w (x - x_0) / W, and x_0 + atan2(sum w sin(x - x_0), sum w cos(x - x_0)) for an angle (the
// same direction and the same resultant length as atan2(S, C) of the unshifted sums).  The differences of float32 values are
// exact in float64, so a constant column -- or a single point -- has mean x_0 and variance 0 exactly, whatever the weights.
//
// Three kernels, no float atomics, everything a workgroup brings decided by blockIdx alone (wave-uniform):
//   (1) moments_mean_kernel: one 256-thread group per ENTRY.  Thread t adds points t, t + 256, ... in order, then wave_sum, then
//       the four waves in order.
//   (2) moments_cov_kernel: one 256-thread group per BLOCK.  The d (d + 1) / 2 <= 136 products of the upper triangle are
//       numbered column by column (p = f (f + 1) / 2 + e, e <= f) and wave w owns p = w, w + 4, ...: at most 34 float64
//       accumulators per lane, indexed at compile time (the wave number is a template argument).  Every wave walks all
//       n points, lane l taking l, l + 64, ...; each of the block's d rows is read coalesced.  The sum of the pair (e, f)
//       depends on n, the two rows and their flags alone, so the diagonal blocks of a pair's matrix are the bits of the
//       variables' own matrices.
//   (3) quantile_kernel: one 256-thread group per ENTRY sorts the float64 keys in dynamic LDS (bitonic, padded with +inf to
//       the next power of two: 8 bytes x padded n, at most 128 KiB) and interpolates by numpy's "linear" rule.
// Hence: two calls give the same bits, and an entry's / a block's results are the same bits alone, repeated, or anywhere in a
// table.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_common.h"

namespace {

using namespace sample_common;

constexpr int MAX_D = NFISAM_MOMENTS_MAX_D;
constexpr int MAX_P = MAX_D * (MAX_D + 1) / 2;        // 136 products of the upper triangle
constexpr int PPW = (MAX_P + 3) / 4;                  // 34 per wave

// grid (n_entries); 256 threads
__global__ void __launch_bounds__(256) moments_mean_kernel(const float* __restrict__ Xt, int x_rows, int n,
                                                           const int32_t* __restrict__ cols, const uint8_t* __restrict__ circular,
                                                           const double* __restrict__ weights, double* __restrict__ mean,
                                                           double* __restrict__ resultant) {
    __shared__ double part[3][4];
    const int e = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int row = cols[e];
    const bool bad = row < 0 || row >= x_rows;                     // never read: row 0 stands in and the entry is NaN
    if (bad) row = 0;
    const bool circ = circular != nullptr && circular[e] != 0;
    const float* __restrict__ x = Xt + (size_t)row * (size_t)n;
    const double x0 = (double)x[0];
    double sw = 0.0, sa = 0.0, sb = 0.0;                           // W, and sum w (x - x0)  |  sum w cos, sum w sin of x - x0
    if (circ) {
        for (int i = threadIdx.x; i < n; i += 256) {
            const double wi = weights != nullptr ? weights[i] : 1.0;
            double sn, cs;
            sincos((double)x[i] - x0, &sn, &cs);
            sw += wi;
            sa = fma(wi, cs, sa);
            sb = fma(wi, sn, sb);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) {
            const double wi = weights != nullptr ? weights[i] : 1.0;
            sw += wi;
            sa = fma(wi, (double)x[i] - x0, sa);
        }
    }
    sw = wave_sum(sw), sa = wave_sum(sa), sb = wave_sum(sb);
    if (lane == 0) part[0][w] = sw, part[1][w] = sa, part[2][w] = sb;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double W = waves_in_order(part[0]), A = waves_in_order(part[1]), B = waves_in_order(part[2]);
        double m, r = (double)NAN;
        if (circ) {
            const double C = A / W, S = B / W;
            m = x0 + atan2(S, C);                                  // [-pi, pi): scipy's circmean(high = pi, low = -pi)
            if (!(m >= -PI && m < PI)) m = wrap_pi(m);             // (in range already: untouched, x_0 itself for one point)
            r = hypot(C, S);
        } else {
            m = x0 + A / W;
        }
        mean[e] = bad ? (double)NAN : m;
        resultant[e] = bad ? (double)NAN : r;
    }
}

// product p of the upper triangle numbered column by column: p = f (f + 1) / 2 + e with e <= f
__host__ __device__ constexpr int tri_f(int p) {
    int f = 0;
    while ((f + 1) * (f + 2) / 2 <= p) ++f;
    return f;
}
__host__ __device__ constexpr int tri_e(int p) { return p - tri_f(p) * (tri_f(p) + 1) / 2; }

template <int W, int K>
struct PairStep {
    static constexpr int P = 4 * K + W, F = tri_f(P), E = tri_e(P);
    static __device__ __forceinline__ void add(double (&acc)[PPW], const double (&r)[MAX_D], double wi, int n_pairs) {
        if (P < n_pairs) acc[K] = fma(wi * r[E], r[F], acc[K]);
        if constexpr (K + 1 < PPW) PairStep<W, K + 1>::add(acc, r, wi, n_pairs);
    }
    static __device__ __forceinline__ void store(const double (&acc)[PPW], double Wsum, int d, int n_pairs, bool bad, int lane,
                                                 double* __restrict__ out) {
        if (P < n_pairs) {
            const double s = wave_sum(acc[K]);
            if (lane == 0) {
                const double v = bad ? (double)NAN : s / Wsum;
                out[E * d + F] = v;
                out[F * d + E] = v;
            }
        }
        if constexpr (K + 1 < PPW) PairStep<W, K + 1>::store(acc, Wsum, d, n_pairs, bad, lane, out);
    }
};

template <int W>
__device__ __forceinline__ void cov_wave(const float* __restrict__ Xt, int n, const int (&rows)[MAX_D], const double (&mu)[MAX_D],
                                         unsigned circ_mask, int d, bool bad, const double* __restrict__ weights, int lane,
                                         double* __restrict__ out) {
    const int n_pairs = d * (d + 1) / 2;
    double acc[PPW];
#pragma unroll
    for (int k = 0; k < PPW; ++k) acc[k] = 0.0;
    double sw = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double wi = weights != nullptr ? weights[i] : 1.0;
        sw += wi;
        double r[MAX_D];
#pragma unroll
        for (int c = 0; c < MAX_D; ++c) {
            r[c] = 0.0;
            if (c < d) {
                const double t = (double)Xt[(size_t)rows[c] * (size_t)n + (size_t)i] - mu[c];
                r[c] = ((circ_mask >> c) & 1u) ? wrap_pi(t) : t;
            }
        }
        PairStep<W, 0>::add(acc, r, wi, n_pairs);
    }
    const double Wsum = wave_total(sw);                            // every wave walks all points: the same bits in all four
    PairStep<W, 0>::store(acc, Wsum, d, n_pairs, bad, lane, out);
}

// grid (n_blocks); 256 threads
__global__ void __launch_bounds__(256) moments_cov_kernel(const nfisam_moment_block* __restrict__ blocks, const float* __restrict__ Xt,
                                                          int x_rows, int n, const int32_t* __restrict__ cols, int n_entries,
                                                          const uint8_t* __restrict__ circular, const double* __restrict__ weights,
                                                          const double* __restrict__ mean, long long cov_count,
                                                          double* __restrict__ cov) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);          // (a scalar: the switch below is a scalar branch)
    const int col_off = blocks[b].col_off, d = blocks[b].d;
    const long long cov_off = blocks[b].cov_off;
    if (d < 1 || d > MAX_D || cov_off < 0 || cov_off + (long long)d * d > cov_count) return;    // no place to write to
    // a block whose entries leave the table is never walked (d_walk rows of row 0 stand in); a row outside the matrix is
    // replaced by row 0: NaN for the whole matrix either way
    bool bad = col_off < 0 || (long long)col_off + d > n_entries;
    int rows[MAX_D];
    double mu[MAX_D];
    unsigned circ_mask = 0;
#pragma unroll
    for (int c = 0; c < MAX_D; ++c) {
        rows[c] = 0, mu[c] = 0.0;
        if (c < d && !bad) {
            const int e = col_off + c;
            int row = cols[e];
            if (row < 0 || row >= x_rows) bad = true, row = 0;
            rows[c] = row;
            mu[c] = mean[e];
            if (circular != nullptr && circular[e] != 0) circ_mask |= 1u << c;
        }
    }
    double* __restrict__ out = cov + cov_off;
    switch (w) {                                                   // (wave-uniform: the wave number picks its products)
        case 0: cov_wave<0>(Xt, n, rows, mu, circ_mask, d, bad, weights, lane, out); break;
        case 1: cov_wave<1>(Xt, n, rows, mu, circ_mask, d, bad, weights, lane, out); break;
        case 2: cov_wave<2>(Xt, n, rows, mu, circ_mask, d, bad, weights, lane, out); break;
        default: cov_wave<3>(Xt, n, rows, mu, circ_mask, d, bad, weights, lane, out); break;
    }
}

// grid (n_entries); 256 threads; dynamic LDS: n_pad doubles
__global__ void __launch_bounds__(256) quantile_kernel(const float* __restrict__ Xt, int x_rows, int n, int n_pad,
                                                       const int32_t* __restrict__ cols, const uint8_t* __restrict__ circular,
                                                       const double* __restrict__ center, const double* __restrict__ probs,
                                                       int n_probs, double* __restrict__ out) {
    extern __shared__ double keys[];                               // [n_pad]
    const int e = blockIdx.x, tid = threadIdx.x;
    int row = cols[e];
    const bool bad = row < 0 || row >= x_rows;
    if (bad) row = 0;
    const bool circ = circular != nullptr && circular[e] != 0;
    const double c0 = circ && center != nullptr ? center[e] : 0.0;
    const float* __restrict__ x = Xt + (size_t)row * (size_t)n;
    for (int i = tid; i < n_pad; i += 256) {
        double k = (double)INFINITY;
        if (i < n) {
            k = (double)x[i];
            if (circ) k = wrap_pi(k - c0);
        }
        keys[i] = k;
    }
    __syncthreads();
    // bitonic sort, ascending: in the stage (k, j) compare-exchange t pairs index i (bit j clear) with i + j
    const int half = n_pad >> 1;
    for (int k = 2; k <= n_pad; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = tid; t < half; t += 256) {
                const int i = 2 * t - (t & (j - 1));
                const double a = keys[i], b = keys[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up && a != b) keys[i] = b, keys[i + j] = a;
            }
            __syncthreads();
        }
    }
    for (int q = tid; q < n_probs; q += 256) {
        const double p = probs[q];
        double v = (double)NAN;
        if (!bad && p >= 0.0 && p <= 1.0) {                        // (a NaN probability fails both comparisons)
            const double h = p * (double)(n - 1);
            int lo = (int)floor(h);
            lo = lo < 0 ? 0 : lo > n - 1 ? n - 1 : lo;
            const int hi = lo + 1 < n ? lo + 1 : n - 1;
            const double frac = h - (double)lo, a = keys[lo], b = keys[hi];
            v = (frac > 0.0 && a != b) ? a + frac * (b - a) : a;    // an integer position, or a tie: the key itself
            if (circ) v += c0;                                     // unwrapped: the ends of an interval stay ordered
        }
        out[(size_t)e * (size_t)n_probs + (size_t)q] = v;
    }
}

int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" int nfisam_sample_moments(const float* Xt, int x_rows, int n, const nfisam_moment_block* blocks,
                                     const nfisam_moment_block* blocks_dev, int n_blocks, const int32_t* cols, int n_entries,
                                     const uint8_t* circular, const double* weights, double* mean, double* resultant, double* cov,
                                     long long cov_count, nfisam_stream_t stream) {
    static_assert(sizeof(nfisam_moment_block) == 16, "nfisam_moment_block is 16 bytes");
    if (Xt == nullptr || blocks == nullptr || blocks_dev == nullptr || cols == nullptr || mean == nullptr || resultant == nullptr ||
        cov == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 1 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535 || cov_count < 1) return NFISAM_ERR_ARG;
    for (int b = 0; b < n_blocks; ++b) {                           // `blocks` is the HOST copy of the table: read here only
        const long long d = blocks[b].d, off = blocks[b].cov_off;
        if (d < 1 || d > MAX_D || off < 0 || off + d * d > cov_count) return NFISAM_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(moments_mean_kernel, dim3((unsigned)n_entries), dim3(256), 0, s, Xt, x_rows, n, cols, circular, weights, mean,
                       resultant);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(moments_cov_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, blocks_dev, Xt, x_rows, n, cols, n_entries,
                           circular, weights, mean, cov_count, cov);
        e = hipGetLastError();
    }
    return launch_status(e);
}

extern "C" int nfisam_sample_quantiles(const float* Xt, int x_rows, int n, const int32_t* cols, int n_entries,
                                       const uint8_t* circular, const double* center, const double* probs, const double* probs_dev,
                                       int n_probs, double* out, nfisam_stream_t stream) {
    if (Xt == nullptr || cols == nullptr || probs == nullptr || probs_dev == nullptr || out == nullptr) return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 1 || n > NFISAM_QUANTILE_MAX_N || n_entries < 1 || n_probs < 1) return NFISAM_ERR_ARG;
    for (int q = 0; q < n_probs; ++q)                              // `probs` is the HOST copy: read here only
        if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return NFISAM_ERR_ARG;
    int n_pad = next_pow2(n);
    if (n_pad < 2) n_pad = 2;
    const size_t lds = (size_t)n_pad * sizeof(double);
    hipError_t e = hipSuccess;
    if (lds > 48 * 1024)                                           // always the fixed maximum: threads with different n cannot
        e = hipFuncSetAttribute((const void*)quantile_kernel,      // lower each other's limit between the set and the launch
                                hipFuncAttributeMaxDynamicSharedMemorySize, NFISAM_QUANTILE_MAX_N * (int)sizeof(double));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(quantile_kernel, dim3((unsigned)n_entries), dim3(256), lds, (hipStream_t)stream, Xt, x_rows, n, n_pad, cols,
                           circular, center, probs_dev, n_probs, out);
        e = hipGetLastError();
    }
    return launch_status(e);
}
