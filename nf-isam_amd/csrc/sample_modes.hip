// sample_modes.hip — where a sample set's hypotheses are: mean-shift mode seeking over many column blocks, then a merge.
//
// The solver's posteriors are multi-modal (a landmark seen by range only, a pose under ambiguous data association); one
// mean and one covariance per variable (sample_summary.hip) put the estimate between the hypotheses.  Here every sample of a
// block climbs the Gaussian kernel density estimate of the block's own samples,
//     k_j(y) = w_j exp(-inv_two_sigma2 * sum_e (scale_e * wrap_e(x_je - y_e))^2),
//     y_e += sum_j k_j(y) wrap_e(x_je - y_e) / sum_j k_j(y)                          (one iteration; a heading is wrapped back),
// until the shift is at most `tol` sigmas or `max_iters` shifts were applied, and the converged points are merged into modes.
// Xt is the COLUMN-major float32 device matrix [x_rows][n] (the walk's St, the layout of sample_common.h); an entry e names
// a row cols[e] of Xt and a block is a run of entries (nfisam_mmd_block).
//
// Numerics: float32 points in; every difference, exponent, sum and division is float64 (the contract of sample_common.h).
// Direct differences, never the Gram identity.  The SHIFT form -- a weighted mean of wrapped differences, not of
// coordinates -- is right across the +-pi seam and leaves a constant column exactly where it is (every difference is exactly
// 0, whatever its scale).  A column with scale 0 does not enter the exponent: it is carried along by the others' weights.
//
// Two launches, no float atomics, everything a workgroup brings decided by blockIdx alone (wave-uniform):
//   (1) modes_ascent_kernel, grid (ceil(n / 64), blocks): a 256-thread group owns 64 starts, one per lane, and ALL their
//       iterations.  Each of the four waves holds the same 64 current points; a pass walks the n points j in chunks of 128
//       staged as doubles in LDS ([17][128]: the block's columns and the weights), wave w taking the chunk's j = 32 w ..
//       32 w + 31 by broadcast reads.  The four partial (shift numerators, denominator) sets meet in LDS and every wave adds
//       them in wave order, so the four copies of a point stay the same bits.  A start that has stopped keeps taking part
//       in the barriers (its lanes compute and discard); the group leaves when all 64 have stopped.  A start takes
//       iters + 1 passes: the last one evaluates the density at the converged point.
//   (2) modes_merge_kernel, one 256-thread group per block: the unlabelled start of largest density (lowest index on ties:
//       a fixed shuffle tree on (density, -index), the four waves in order) founds a mode; every unlabelled start within
//       `merge` sigmas of it takes its label; until none is left or max_modes exist.  The mode table lives in LDS.
// The sum over j of a start is: per wave its j ascending, then waves 0..3 -- an order that depends on n alone.  Hence two
// calls give the same bits, and a block's results are the same bits alone, repeated, or anywhere in a table.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

constexpr int MAX_D = NFISAM_MODES_MAX_D;
constexpr int MAX_MODES = NFISAM_MODES_MAX_MODES;
constexpr int SPG = 64;           // starts per group: one per lane, the same 64 in each of the four waves
constexpr int JT = 128;           // points j per staged chunk
constexpr int JPW = JT / 4;       // ... of which a wave takes 32
constexpr int ROWS = MAX_D + 1;   // staged rows: the columns and the weights | partial sums: the numerators and the denominator

// sum of w over all points (n for NULL weights): thread t adds t, t + 256, ... in order, wave_sum, the four waves in order.
// Every thread of the group returns the same bits.  `part` is 4 doubles of LDS; two barriers.
__device__ __forceinline__ double group_weight_sum(const double* __restrict__ weights, int n, double* part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += weights != nullptr ? weights[i] : 1.0;
    s = wave_sum(s);
    if (lane == 0) part[w] = s;
    __syncthreads();
    const double W = waves_in_order(part);
    __syncthreads();
    return W;
}

// what a block brings, the same in every thread of its groups
struct BlockHead {
    int col_off, d;
    double inv;
    bool bad;                      // entries outside the tables, a row outside the matrix, d outside 1..16: never walked
};

__device__ __forceinline__ BlockHead block_head(const nfisam_mmd_block* __restrict__ blocks, int b, const int32_t* __restrict__ cols,
                                                int n_entries, int x_rows) {
    BlockHead h;
    h.col_off = blocks[b].col_off, h.d = blocks[b].d, h.inv = blocks[b].inv_two_sigma2;
    h.bad = h.d < 1 || h.d > MAX_D || h.col_off < 0 || (long long)h.col_off + h.d > n_entries;
    if (!h.bad)
        for (int c = 0; c < h.d; ++c) {
            const int row = cols[h.col_off + c];
            if (row < 0 || row >= x_rows) h.bad = true;
        }
    return h;
}

// all iterations of the group's 64 starts, for a block of d <= DM columns (DM picks the unrolled width; columns c >= d of
// the register arrays are never touched)
template <int DM>
__device__ __forceinline__ void ascend(const BlockHead h, const float* __restrict__ Xt, int n, const int* row_s, const double* sc_s,
                                       const uint8_t* __restrict__ wrap, const double* __restrict__ weights, int max_iters,
                                       double tol2, double W, double (*xs)[JT], double (*part)[ROWS][SPG], double* __restrict__ pos,
                                       double* __restrict__ dens, int32_t* __restrict__ iters) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
    const int d = h.d, b = blockIdx.y;
    const double inv = h.inv;
    const int i = blockIdx.x * SPG + lane;

    // the block's rows and scales come from LDS (`row_s`, `sc_s`): as vector registers they leave the scalar file to the loop
    double sc[DM], y[DM];
    unsigned wrap_mask = 0;
#pragma unroll
    for (int c = 0; c < DM; ++c) {
        sc[c] = 0.0, y[c] = 0.0;
        if (c < d) {
            sc[c] = sc_s[c];
            if (wrap != nullptr && wrap[h.col_off + c] != 0) wrap_mask |= 1u << c;
            if (i < n) y[c] = (double)Xt[(size_t)row_s[c] * (size_t)n + (size_t)i];
        }
    }

    bool done = i >= n, final_pass = false, capped = false;
    int it = 0;
    double density = 0.0;
    const bool stage_once = n <= JT;                               // one chunk: it stays in LDS for every pass

    for (int pass = 0;; ++pass) {
        double acc[DM], den = 0.0;
#pragma unroll
        for (int c = 0; c < DM; ++c) acc[c] = 0.0;

        for (int j0 = 0; j0 < n; j0 += JT) {
            if (!stage_once || pass == 0) {
                __syncthreads();                                   // the previous chunk has been read
                if (tid < JT) {
                    const int j = j0 + tid;
                    const bool in = j < n;
                    for (int c = 0; c < d; ++c)
                        xs[c][tid] = in ? (double)Xt[(size_t)row_s[c] * (size_t)n + (size_t)j] : 0.0;
                    xs[MAX_D][tid] = in ? (weights != nullptr ? weights[j] : 1.0) : 0.0;
                }
                __syncthreads();
            }
            const int cnt = min(JT, n - j0);
            const int jb = w * JPW, je = min(jb + JPW, cnt);
            for (int jl = jb; jl < je; ++jl) {
                double diff[DM], q = 0.0;
#pragma unroll
                for (int c = 0; c < DM; ++c) {
                    diff[c] = 0.0;
                    if (c < d) {
                        double t = xs[c][jl] - y[c];
                        if ((wrap_mask >> c) & 1u) t = wrap_pi_near(t);
                        diff[c] = t;
                        const double u = sc[c] * t;
                        q = fma(u, u, q);
                    }
                }
                const double k = xs[MAX_D][jl] * exp(-inv * q);
                den += k;
#pragma unroll
                for (int c = 0; c < DM; ++c)
                    if (c < d) acc[c] = fma(k, diff[c], acc[c]);
            }
        }

        // the four partial sets, added in wave order by every wave: the four copies of y stay the same bits
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < d) part[w][c][lane] = acc[c];
        part[w][MAX_D][lane] = den;
        __syncthreads();
        den = ((part[0][MAX_D][lane] + part[1][MAX_D][lane]) + part[2][MAX_D][lane]) + part[3][MAX_D][lane];
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < d) acc[c] = ((part[0][c][lane] + part[1][c][lane]) + part[2][c][lane]) + part[3][c][lane];

        if (!done) {
            if (final_pass) {
                density = den / W, done = true;
            } else if (!(den > 0.0)) {                             // a zero-weight start out of reach of every weighted point
                density = den == 0.0 ? 0.0 : (double)NAN, done = true;
            } else {
                double crit = 0.0;
#pragma unroll
                for (int c = 0; c < DM; ++c)
                    if (c < d) {
                        const double delta = acc[c] / den;
                        double v = y[c] + delta;
                        if ((wrap_mask >> c) & 1u) v = wrap_pi_near(v);
                        y[c] = v;
                        const double s = sc[c] * delta;
                        crit = fma(s, s, crit);
                    }
                ++it;
                if (2.0 * inv * crit <= tol2) final_pass = true;
                else if (it >= max_iters) final_pass = true, capped = true;
            }
        }
        if (__syncthreads_and(done ? 1 : 0)) break;                // (also: the partial sums have been read)
    }

    if (w == 0 && i < n) {
#pragma unroll
        for (int c = 0; c < DM; ++c)
            if (c < d) pos[(size_t)(h.col_off + c) * (size_t)n + (size_t)i] = y[c];
        dens[(size_t)b * (size_t)n + (size_t)i] = density;
        iters[(size_t)b * (size_t)n + (size_t)i] = capped ? -it : it;
    }
}

// grid (ceil(n / 64), n_blocks); 256 threads
__global__ void __launch_bounds__(256) modes_ascent_kernel(const nfisam_mmd_block* __restrict__ blocks, const float* __restrict__ Xt,
                                                           int x_rows, int n, const int32_t* __restrict__ cols, int n_entries,
                                                           const double* __restrict__ scale, const uint8_t* __restrict__ wrap,
                                                           const double* __restrict__ weights, int max_iters, double tol2,
                                                           double* __restrict__ pos, double* __restrict__ dens,
                                                           int32_t* __restrict__ iters) {
    __shared__ double xs[ROWS][JT];                                // 17 KiB: the staged chunk
    __shared__ double part[4][ROWS][SPG];                          // 34 KiB: the waves' partial sums
    __shared__ double wpart[4], sc_s[MAX_D];
    __shared__ int row_s[MAX_D];
    const int b = blockIdx.y;
    const BlockHead h = block_head(blocks, b, cols, n_entries, x_rows);
    if (h.bad) {                                                   // (the whole group: no barrier is left waiting)
        const int i = blockIdx.x * SPG + (int)threadIdx.x;
        if (threadIdx.x < SPG && i < n) {
            if (h.d >= 1 && h.d <= MAX_D)
                for (int c = 0; c < h.d; ++c) {
                    const long long e = (long long)h.col_off + c;
                    if (e >= 0 && e < n_entries) pos[(size_t)e * (size_t)n + (size_t)i] = (double)NAN;
                }
            dens[(size_t)b * (size_t)n + (size_t)i] = (double)NAN;
            iters[(size_t)b * (size_t)n + (size_t)i] = 0;
        }
        return;
    }
    if (threadIdx.x < MAX_D) {
        const bool in = (int)threadIdx.x < h.d;
        row_s[threadIdx.x] = in ? cols[h.col_off + threadIdx.x] : 0;
        sc_s[threadIdx.x] = in ? (scale != nullptr ? scale[h.col_off + threadIdx.x] : 1.0) : 0.0;
    }
    const double W = group_weight_sum(weights, n, wpart);          // (its barriers also publish row_s and sc_s)
    if (h.d <= 2) ascend<2>(h, Xt, n, row_s, sc_s, wrap, weights, max_iters, tol2, W, xs, part, pos, dens, iters);
    else if (h.d <= 3) ascend<3>(h, Xt, n, row_s, sc_s, wrap, weights, max_iters, tol2, W, xs, part, pos, dens, iters);
    else if (h.d <= 6) ascend<6>(h, Xt, n, row_s, sc_s, wrap, weights, max_iters, tol2, W, xs, part, pos, dens, iters);
    else ascend<MAX_D>(h, Xt, n, row_s, sc_s, wrap, weights, max_iters, tol2, W, xs, part, pos, dens, iters);
}

// is (bd, bi) ahead of (ad, ai) in the (density, -index) order?  An index < 0 is "none".
__device__ __forceinline__ bool ahead(double ad, int ai, double bd, int bi) {
    return bi >= 0 && (ai < 0 || bd > ad || (bd == ad && bi < ai));
}

// grid (n_blocks); 256 threads
__global__ void __launch_bounds__(256) modes_merge_kernel(const nfisam_mmd_block* __restrict__ blocks, int x_rows, int n,
                                                          const int32_t* __restrict__ cols, int n_entries,
                                                          const double* __restrict__ scale, const uint8_t* __restrict__ wrap,
                                                          const double* __restrict__ weights, double merge2, int max_modes,
                                                          const double* __restrict__ pos, const double* __restrict__ dens,
                                                          int32_t* __restrict__ labels, int32_t* __restrict__ n_modes,
                                                          double* __restrict__ mode_pos, double* __restrict__ mode_dens,
                                                          double* __restrict__ mode_mass, int32_t* __restrict__ unlabelled) {
    __shared__ double tab[MAX_MODES][MAX_D];                       // the mode table
    __shared__ double tab_dens[MAX_MODES], tab_mass[MAX_MODES];
    __shared__ double sc_s[MAX_D];
    __shared__ int wrap_s[MAX_D];
    __shared__ double wd[4], wm[4];
    __shared__ int wi[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const BlockHead h = block_head(blocks, b, cols, n_entries, x_rows);
    int32_t* __restrict__ lab = labels + (size_t)b * (size_t)n;
    const double* __restrict__ dn = dens + (size_t)b * (size_t)n;
    double* __restrict__ mp = mode_pos + (size_t)b * (size_t)max_modes * MAX_D;
    for (int i = tid; i < n; i += 256) lab[i] = -1;                // (a thread reads back only what it wrote itself)
    if (h.bad) {
        for (int k = tid; k < max_modes * MAX_D; k += 256) mp[k] = (double)NAN;
        for (int k = tid; k < max_modes; k += 256)
            mode_dens[(size_t)b * max_modes + k] = (double)NAN, mode_mass[(size_t)b * max_modes + k] = (double)NAN;
        if (tid == 0) n_modes[b] = 0, unlabelled[b] = n;
        return;
    }
    const int d = h.d;
    if (tid < MAX_D) {
        const bool in = tid < d;
        sc_s[tid] = in ? (scale != nullptr ? scale[h.col_off + tid] : 1.0) : 0.0;
        wrap_s[tid] = in && wrap != nullptr && wrap[h.col_off + tid] != 0;
    }
    const double W = group_weight_sum(weights, n, wd);             // (its barriers also publish sc_s and wrap_s)
    const double* __restrict__ p0 = pos + (size_t)h.col_off * (size_t)n;

    int m = 0;
    for (; m < max_modes; ++m) {
        // the unlabelled start of largest density, lowest index on ties
        double bd = 0.0;
        int bi = -1;
        for (int i = tid; i < n; i += 256) {
            const double v = dn[i];
            if (lab[i] < 0 && v == v && ahead(bd, bi, v, i)) bd = v, bi = i;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_down(bd, off, 64);
            const int oi = __shfl_down(bi, off, 64);
            if (ahead(bd, bi, od, oi)) bd = od, bi = oi;
        }
        if (lane == 0) wd[w] = bd, wi[w] = bi;
        __syncthreads();
        bd = wd[0], bi = wi[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (ahead(bd, bi, wd[k], wi[k])) bd = wd[k], bi = wi[k];
        if (bi < 0) break;                                         // (the same in every thread) nothing left to label
        if (tid < MAX_D) tab[m][tid] = tid < d ? p0[(size_t)tid * (size_t)n + (size_t)bi] : (double)NAN;
        if (tid == 0) tab_dens[m] = bd;
        __syncthreads();
        // every unlabelled start within `merge` sigmas of it
        double mass = 0.0;
        for (int i = tid; i < n; i += 256) {
            if (lab[i] >= 0) continue;
            double q = 0.0;
            for (int c = 0; c < d; ++c) {
                double t = p0[(size_t)c * (size_t)n + (size_t)i] - tab[m][c];
                if (wrap_s[c]) t = wrap_pi_near(t);
                const double u = sc_s[c] * t;
                q = fma(u, u, q);
            }
            if (2.0 * h.inv * q <= merge2) {
                lab[i] = m;
                mass += weights != nullptr ? weights[i] : 1.0;
            }
        }
        mass = wave_sum(mass);
        if (lane == 0) wm[w] = mass;
        __syncthreads();
        if (tid == 0) tab_mass[m] = waves_in_order(wm) / W;
    }
    __syncthreads();
    int left = 0;
    for (int i = tid; i < n; i += 256) left += lab[i] < 0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) left += __shfl_down(left, off, 64);
    if (lane == 0) wi[w] = left;
    for (int k = tid; k < max_modes * MAX_D; k += 256) mp[k] = k / MAX_D < m ? tab[k / MAX_D][k % MAX_D] : (double)NAN;
    for (int k = tid; k < max_modes; k += 256) {
        mode_dens[(size_t)b * max_modes + k] = k < m ? tab_dens[k] : (double)NAN;
        mode_mass[(size_t)b * max_modes + k] = k < m ? tab_mass[k] : (double)NAN;
    }
    __syncthreads();
    if (tid == 0) n_modes[b] = m, unlabelled[b] = wi[0] + wi[1] + wi[2] + wi[3];
}

}  // namespace

namespace {

bool table_ok(const nfisam_mmd_block* blocks, int n_blocks) { return check_block_table(blocks, n_blocks, MAX_D); }

bool merge_args_ok(double merge, int max_modes) {
    return merge > 0.0 && isfinite(merge) && max_modes >= 1 && max_modes <= MAX_MODES;
}

hipError_t launch_merge(const nfisam_mmd_block* blocks_dev, int n_blocks, int x_rows, int n, const int32_t* cols, int n_entries,
                        const double* scale, const uint8_t* wrap, const double* weights, double merge, int max_modes,
                        const double* pos, const double* dens, int32_t* labels, int32_t* n_modes, double* mode_pos,
                        double* mode_dens, double* mode_mass, int32_t* unlabelled, hipStream_t s) {
    hipLaunchKernelGGL(modes_merge_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, blocks_dev, x_rows, n, cols, n_entries, scale,
                       wrap, weights, merge * merge, max_modes, pos, dens, labels, n_modes, mode_pos, mode_dens, mode_mass,
                       unlabelled);
    return hipGetLastError();
}

}  // namespace

extern "C" int nfisam_sample_modes(const float* Xt, int x_rows, int n, const nfisam_mmd_block* blocks,
                                   const nfisam_mmd_block* blocks_dev, int n_blocks, const int32_t* cols, int n_entries,
                                   const double* scale, const uint8_t* wrap, const double* weights, int max_iters, double tol,
                                   double merge, int max_modes, double* pos, double* dens, int32_t* iters, int32_t* labels,
                                   int32_t* n_modes, double* mode_pos, double* mode_dens, double* mode_mass, int32_t* unlabelled,
                                   nfisam_stream_t stream) {
    if (Xt == nullptr || blocks == nullptr || blocks_dev == nullptr || cols == nullptr || pos == nullptr || dens == nullptr ||
        iters == nullptr || labels == nullptr || n_modes == nullptr || mode_pos == nullptr || mode_dens == nullptr ||
        mode_mass == nullptr || unlabelled == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 0 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535) return NFISAM_ERR_ARG;
    if (max_iters < 1 || !(tol >= 0.0) || !isfinite(tol) || !merge_args_ok(merge, max_modes)) return NFISAM_ERR_ARG;
    if (!table_ok(blocks, n_blocks)) return NFISAM_ERR_ARG;
    if (n == 0) return NFISAM_OK;                                  // nothing to climb from: nothing is touched
    hipStream_t s = (hipStream_t)stream;
    const unsigned groups = (unsigned)(((long long)n + SPG - 1) / SPG);
    hipLaunchKernelGGL(modes_ascent_kernel, dim3(groups, (unsigned)n_blocks), dim3(256), 0, s, blocks_dev, Xt, x_rows, n, cols,
                       n_entries, scale, wrap, weights, max_iters, tol * tol, pos, dens, iters);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = launch_merge(blocks_dev, n_blocks, x_rows, n, cols, n_entries, scale, wrap, weights, merge, max_modes, pos, dens, labels,
                         n_modes, mode_pos, mode_dens, mode_mass, unlabelled, s);
    return launch_status(e);
}

// the second launch alone: converged points and densities of an earlier nfisam_sample_modes call merged again, with another
// radius or another max_modes, without climbing again
extern "C" int nfisam_sample_modes_merge(int x_rows, int n, const nfisam_mmd_block* blocks, const nfisam_mmd_block* blocks_dev,
                                         int n_blocks, const int32_t* cols, int n_entries, const double* scale, const uint8_t* wrap,
                                         const double* weights, double merge, int max_modes, const double* pos, const double* dens,
                                         int32_t* labels, int32_t* n_modes, double* mode_pos, double* mode_dens, double* mode_mass,
                                         int32_t* unlabelled, nfisam_stream_t stream) {
    if (blocks == nullptr || blocks_dev == nullptr || cols == nullptr || pos == nullptr || dens == nullptr || labels == nullptr ||
        n_modes == nullptr || mode_pos == nullptr || mode_dens == nullptr || mode_mass == nullptr || unlabelled == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 0 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535) return NFISAM_ERR_ARG;
    if (!merge_args_ok(merge, max_modes) || !table_ok(blocks, n_blocks)) return NFISAM_ERR_ARG;
    if (n == 0) return NFISAM_OK;
    const hipError_t e = launch_merge(blocks_dev, n_blocks, x_rows, n, cols, n_entries, scale, wrap, weights, merge, max_modes, pos,
                                      dens, labels, n_modes, mode_pos, mode_dens, mode_mass, unlabelled, (hipStream_t)stream);
    return launch_status(e);
}
