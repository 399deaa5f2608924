// sample_trajectory.hip — trajectory error of every posterior sample against ground truth: aligned ATE and RPE.
//
// The reference grades ONE trajectory, the posterior mean, on the host: it copies the sample matrix out, takes mean(0),
// aligns it to the truth with `kabsch_umeyama` (src/utils/Functions.py:53-71: an SVD) and reports the RMSE of what is left
// (example/slam/plaza_dataset/plaza_traj_performance_plot.py:112-114,196-198,282-293).  Every row of the walk's matrix is one
// complete trajectory, and on a multi-modal posterior the mean is none of them.  Here every sample is aligned and graded where
// the tree walk wrote it: Xt is the COLUMN-major float32 device matrix [x_rows][n] (the layout of sample_common.h), an entry
// of the table names the rows of one pose or landmark and holds its float64 truth, and a lane carries one sample.
//
// THE ALIGNMENT, in closed form for the plane (what the SVD route gives with S = diag(1, d)).  Over the entries with flag bit 0,
// with a', b' the truth and the sample about their centroids (the truth's, a_bar, is the host's: it is the same for every
// sample):
//     dot = sum a'.b',  cross = sum (a'_y b'_x - a'_x b'_y),  g = hypot(dot, cross),  theta = atan2(cross, dot)
//     none: theta = 0, c = 1, t = 0;   rigid: c = 1;   similarity: c = g / sum |b'|^2;   t = a_bar - c R(theta) b_bar.
// With `reflect` the improper fit R(phi) diag(1, -1) is tried as well -- dot- = sum (a'_x b'_x - a'_y b'_y),
// cross- = sum (a'_x b'_y + a'_y b'_x), phi = atan2(cross-, dot-) -- and taken when its trace hypot(dot-, cross-) is the larger;
// a heading h then maps to phi - h.  Fixed rule for the degenerate fits: g == 0 (one aligned entry, coincident points) gives
// theta = 0; sum |b'|^2 == 0 gives c = 1.
// Every step is two-pass: the centroid first, then products of the centred coordinates, then the residuals
// a - (c R b + t) in a third sweep -- never sum x^2 - (sum x)^2 on coordinates of 100 m.
//
// Numerics: float32 points in; every difference, product, transcendental and sum is float64 (the contract of
// sample_common.h).  No float atomics.
//
// THE LAUNCH.  traj_error_kernel: one 256-thread group per tile of 64 samples.  Lane l of EVERY wave carries sample
// 64 tile + l; wave w takes the entries w, w + 4, ... in ascending order; the four waves' partial sums of a sample meet in LDS
// and are added in wave order (waves_in_order), by every wave alike, so all four hold the same transform.  The table is read
// at a wave-uniform index: every branch on it is a scalar branch.  A sample's sums are taken in an order that P and the table
// fix: its results depend on its own column alone, not on n, and two calls give the same bits.
// Per ENTRY, sum_i w_i |r_i|^2 needs the other direction: a wave_sum over the tile's 64 lanes per entry goes to
// scratch[tile][entry] (and the tile's sum of w to scratch[tile][P]); traj_entry_reduce_kernel then adds the tiles in
// ascending order, one thread per entry.
// traj_rpe_kernel: a group per (tile of 64 samples, slot); wave w takes the pairs w, w + 4, ... of the table and skips those
// of other slots (wave-uniform), so one launch serves every stride.
// A NaN or infinite coordinate of a sample, in any entry, makes every output of THAT sample NaN (the error entry; the RPE
// entry: the slots whose pairs read it), and with it the per-entry sums, which add over the samples; no other sample changes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_common.h"

namespace {

using namespace sample_common;

struct Tile {
    int lane, w;
    bool live;
    size_t i;                                          // the lane's sample (the last one stands in past the end: never stored)
};

__device__ __forceinline__ Tile tile_of(int n) {
    Tile t;
    t.lane = threadIdx.x & 63;
    t.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // (a scalar: the entry loops below are scalar loops)
    const long long i = (long long)blockIdx.x * 64 + t.lane;
    t.live = i < (long long)n;
    t.i = t.live ? (size_t)i : (size_t)(n - 1);
    return t;
}

// one coordinate of the lane's sample; a row outside the matrix is never read: row 0 stands in and the value is NaN
__device__ __forceinline__ double coord(const float* __restrict__ Xt, int x_rows, size_t n, int row, size_t i) {
    const bool bad = row < 0 || row >= x_rows;
    const double v = (double)Xt[(size_t)(bad ? 0 : row) * n + i];
    return bad ? (double)NAN : v;
}

// grid (tiles of 64 samples); 256 threads
__global__ void __launch_bounds__(256) traj_error_kernel(const float* __restrict__ Xt, int x_rows, int n,
                                                         const nfisam_traj_entry* __restrict__ ent, int P, int mode, int reflect,
                                                         double abar_x, double abar_y, double n_align,
                                                         const double* __restrict__ weights, double* __restrict__ out,
                                                         int32_t* __restrict__ iout, double* __restrict__ scratch) {
    __shared__ double part[5][64][4];
    const Tile t = tile_of(n);
    const int lane = t.lane, w = t.w;
    const size_t N = (size_t)n, i = t.i;

    // sweep 1: the sample's centroid over the aligned entries; 0 * every coordinate, which is NaN for a NaN or an infinity
    double sx = 0.0, sy = 0.0, poison = 0.0;
#pragma unroll 4
    for (int e = w; e < P; e += 4) {                               // (the unroll keeps the sums in order; measured: no gain)
        const nfisam_traj_entry E = ent[e];
        const double bx = coord(Xt, x_rows, N, E.col_x, i), by = coord(Xt, x_rows, N, E.col_y, i);
        poison = fma(0.0, bx, poison);
        poison = fma(0.0, by, poison);
        if (E.col_th >= 0) poison = fma(0.0, coord(Xt, x_rows, N, E.col_th, i), poison);
        if (E.flags & NFISAM_TRAJ_ALIGNED) sx += bx, sy += by;
    }
    part[0][lane][w] = sx, part[1][lane][w] = sy, part[2][lane][w] = poison;
    __syncthreads();
    const double bbar_x = waves_in_order(part[0][lane]) / n_align, bbar_y = waves_in_order(part[1][lane]) / n_align;
    poison = waves_in_order(part[2][lane]);
    __syncthreads();

    // sweep 2: the sums of the closed form, then the transform -- in every wave, from the same partial sums in the same order
    double theta = 0.0, c = 1.0, tx = 0.0, ty = 0.0, cs = 1.0, sn = 0.0, flip = 1.0;
    int refl = 0;
    if (mode != NFISAM_TRAJ_ALIGN_NONE) {
        double dot = 0.0, crs = 0.0, dotm = 0.0, crsm = 0.0, sbb = 0.0;
#pragma unroll 4
        for (int e = w; e < P; e += 4) {
            const nfisam_traj_entry E = ent[e];
            if (!(E.flags & NFISAM_TRAJ_ALIGNED)) continue;
            const double ax = E.ax - abar_x, ay = E.ay - abar_y;
            const double bx = coord(Xt, x_rows, N, E.col_x, i) - bbar_x, by = coord(Xt, x_rows, N, E.col_y, i) - bbar_y;
            dot = fma(ay, by, fma(ax, bx, dot));
            crs = fma(-ax, by, fma(ay, bx, crs));
            dotm = fma(-ay, by, fma(ax, bx, dotm));
            crsm = fma(ay, bx, fma(ax, by, crsm));
            sbb = fma(by, by, fma(bx, bx, sbb));
        }
        part[0][lane][w] = dot, part[1][lane][w] = crs, part[2][lane][w] = dotm, part[3][lane][w] = crsm, part[4][lane][w] = sbb;
        __syncthreads();
        dot = waves_in_order(part[0][lane]), crs = waves_in_order(part[1][lane]);
        dotm = waves_in_order(part[2][lane]), crsm = waves_in_order(part[3][lane]);
        sbb = waves_in_order(part[4][lane]);
        __syncthreads();
        double g = hypot(dot, crs);
        if (reflect) {
            const double gm = hypot(dotm, crsm);
            if (gm > g) refl = 1, flip = -1.0, g = gm, dot = dotm, crs = crsm;
        }
        theta = g == 0.0 ? 0.0 : atan2(crs, dot);
        if (mode == NFISAM_TRAJ_ALIGN_SIMILARITY) c = sbb == 0.0 ? 1.0 : g / sbb;
        sincos(theta, &sn, &cs);
        const double fy = flip * bbar_y;
        tx = abar_x - c * (cs * bbar_x - sn * fy);
        ty = abar_y - c * (sn * bbar_x + cs * fy);
    }

    // sweep 3: residuals a - (c R b + t)
    const double wi = !t.live ? 0.0 : weights != nullptr ? weights[i] : 1.0;
    double sse_t = 0.0, sse_l = 0.0, sse_h = 0.0, rmax = -1.0;
    int imax = -1;
    double* __restrict__ tile_sums = scratch + (size_t)blockIdx.x * (size_t)(P + 1);
#pragma unroll 4
    for (int e = w; e < P; e += 4) {
        const nfisam_traj_entry E = ent[e];
        const double bx = coord(Xt, x_rows, N, E.col_x, i), by = flip * coord(Xt, x_rows, N, E.col_y, i);
        const double rx = E.ax - (c * (cs * bx - sn * by) + tx), ry = E.ay - (c * (sn * bx + cs * by) + ty);
        const double r2 = fma(ry, ry, rx * rx);
        if (E.flags & NFISAM_TRAJ_LANDMARK) {
            sse_l += r2;
        } else {
            sse_t += r2;
            if (r2 > rmax) rmax = r2, imax = e;
        }
        if (E.col_th >= 0) {
            const double bth = coord(Xt, x_rows, N, E.col_th, i);
            const double h = wrap_pi((refl ? theta - bth : bth + theta) - E.ath);
            sse_h = fma(h, h, sse_h);
        }
        const double v = wave_sum(t.live ? wi * (r2 + poison) : 0.0);
        if (lane == 0) tile_sums[e] = v;
    }
    if (w == 0) {
        const double v = wave_sum(wi);
        if (lane == 0) tile_sums[P] = v;
    }
    part[0][lane][w] = sse_t, part[1][lane][w] = sse_l, part[2][lane][w] = sse_h, part[3][lane][w] = rmax;
    part[4][lane][w] = (double)imax;
    __syncthreads();
    if (w != 0 || !t.live) return;
    sse_t = waves_in_order(part[0][lane]), sse_l = waves_in_order(part[1][lane]), sse_h = waves_in_order(part[2][lane]);
    rmax = part[3][lane][0], imax = (int)part[4][lane][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {                                  // the largest residual; of equal ones the first entry
        const double r = part[3][lane][k];
        const int ix = (int)part[4][lane][k];
        if (r > rmax || (r == rmax && ix >= 0 && ix < imax)) rmax = r, imax = ix;
    }
    const bool nan = poison != poison || theta != theta;
    static_assert(NFISAM_TRAJ_OUT_ROWS == 8, "out has eight rows");
    out[0 * N + i] = theta + poison;
    out[1 * N + i] = c + poison;
    out[2 * N + i] = tx + poison;
    out[3 * N + i] = ty + poison;
    out[4 * N + i] = sse_t + poison;
    out[5 * N + i] = sse_l + poison;
    out[6 * N + i] = sse_h + poison;
    out[7 * N + i] = (nan || imax < 0) ? (double)NAN : sqrt(rmax);
    iout[i] = nan ? 0 : refl;
    iout[N + i] = nan ? -1 : imax;
}

// grid (ceil((P + 1) / 256)); 256 threads: sums[e] = the tiles' partial sums of entry e in ascending tile order; sums[P] = sum w
__global__ void __launch_bounds__(256) traj_entry_reduce_kernel(const double* __restrict__ scratch, int n_tiles, int P,
                                                                double* __restrict__ sums) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e > P) return;
    double s = 0.0;
    for (int t = 0; t < n_tiles; ++t) s += scratch[(size_t)t * (size_t)(P + 1) + (size_t)e];
    sums[e] = s;
}

// the relative pose of entry j seen from entry i and its heading difference, from float64 coordinates
__device__ __forceinline__ void relative_pose(double xi, double yi, double thi, double xj, double yj, double thj, double& dx,
                                              double& dy, double& dth) {
    double sn, cs;
    sincos(thi, &sn, &cs);
    const double ex = xj - xi, ey = yj - yi;
    dx = fma(sn, ey, cs * ex);                                     // R(-th_i) (p_j - p_i)
    dy = fma(cs, ey, -(sn * ex));
    dth = wrap_pi(thj - thi);
}

// grid (tiles of 64 samples, slots); 256 threads
__global__ void __launch_bounds__(256) traj_rpe_kernel(const float* __restrict__ Xt, int x_rows, int n,
                                                       const nfisam_traj_entry* __restrict__ ent, int P,
                                                       const nfisam_traj_pair* __restrict__ pairs, int n_pairs,
                                                       double* __restrict__ out) {
    __shared__ double part[2][64][4];
    const Tile t = tile_of(n);
    const int lane = t.lane, w = t.w, slot = blockIdx.y;
    const size_t N = (size_t)n, i = t.i;
    double st = 0.0, sr = 0.0;
    for (int p = w; p < n_pairs; p += 4) {
        const nfisam_traj_pair Q = pairs[p];
        if (Q.slot != slot) continue;
        if (Q.i < 0 || Q.i >= P || Q.j < 0 || Q.j >= P) {          // (the device copy is not trusted: NaN, nothing read)
            st = sr = (double)NAN;
            continue;
        }
        const nfisam_traj_entry A = ent[Q.i], B = ent[Q.j];
        double ex, ey, eth, fx, fy, fth;
        relative_pose(coord(Xt, x_rows, N, A.col_x, i), coord(Xt, x_rows, N, A.col_y, i), coord(Xt, x_rows, N, A.col_th, i),
                      coord(Xt, x_rows, N, B.col_x, i), coord(Xt, x_rows, N, B.col_y, i), coord(Xt, x_rows, N, B.col_th, i), ex,
                      ey, eth);
        relative_pose(A.ax, A.ay, A.ath, B.ax, B.ay, B.ath, fx, fy, fth);
        const double ux = ex - fx, uy = ey - fy, ut = wrap_pi(eth - fth);
        st = fma(uy, uy, fma(ux, ux, st));
        sr = fma(ut, ut, sr);
    }
    part[0][lane][w] = st, part[1][lane][w] = sr;
    __syncthreads();
    if (w != 0 || !t.live) return;
    double* __restrict__ o = out + (size_t)slot * 2 * N;
    o[i] = waves_in_order(part[0][lane]);
    o[N + i] = waves_in_order(part[1][lane]);
}

bool is_finite(double v) { return v - v == 0.0; }

// Neumaier's compensated sum (host): the error of the running sum is carried along and added at the end
struct Compensated {
    volatile double s = 0.0, c = 0.0;                  // (volatile: the compensation must not be reassociated away)
    void add(double v) {
        const double t = s + v;
        c += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
        s = t;
    }
    double value() const { return s + c; }
};

// the host copy of the entry table: rows inside the matrix, finite truth, no flag beyond the two; -> the number of aligned entries
int check_entries(const nfisam_traj_entry* entries, int P, int x_rows) {
    int aligned = 0;
    for (int e = 0; e < P; ++e) {
        const nfisam_traj_entry& E = entries[e];
        if (E.col_x < 0 || E.col_x >= x_rows || E.col_y < 0 || E.col_y >= x_rows || E.col_th < -1 || E.col_th >= x_rows) return -1;
        if ((E.flags & ~(NFISAM_TRAJ_ALIGNED | NFISAM_TRAJ_LANDMARK)) != 0) return -1;
        if (!is_finite(E.ax) || !is_finite(E.ay) || (E.col_th >= 0 && !is_finite(E.ath))) return -1;
        aligned += (E.flags & NFISAM_TRAJ_ALIGNED) != 0;
    }
    return aligned;
}

}  // namespace

extern "C" size_t nfisam_sample_trajectory_scratch_count(int n, int P) {
    if (n < 1 || P < 1) return 0;
    return (size_t)((n + 63) / 64) * (size_t)(P + 1);
}

extern "C" int nfisam_sample_trajectory_error(const float* Xt, int x_rows, int n, const nfisam_traj_entry* entries,
                                              const nfisam_traj_entry* entries_dev, int P, int mode, int reflect,
                                              const double* weights, double* out, int32_t* iout, double* entry_sums,
                                              double* scratch, nfisam_stream_t stream) {
    static_assert(sizeof(nfisam_traj_entry) == 40, "nfisam_traj_entry is 40 bytes");
    if (Xt == nullptr || entries == nullptr || entries_dev == nullptr || out == nullptr || iout == nullptr ||
        entry_sums == nullptr || scratch == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 1 || P < 1) return NFISAM_ERR_ARG;
    if (mode != NFISAM_TRAJ_ALIGN_NONE && mode != NFISAM_TRAJ_ALIGN_RIGID && mode != NFISAM_TRAJ_ALIGN_SIMILARITY)
        return NFISAM_ERR_ARG;
    const int aligned = check_entries(entries, P, x_rows);         // `entries` is the HOST copy of the table: read here only
    if (aligned < 0 || (mode != NFISAM_TRAJ_ALIGN_NONE && aligned < 1)) return NFISAM_ERR_ARG;
    // the truth's centroid over the aligned entries, in entry order with a compensated sum: one rounding of the sum, one of the
    // division, whatever P
    double abar_x = 0.0, abar_y = 0.0;
    if (aligned > 0) {
        Compensated sx, sy;
        for (int e = 0; e < P; ++e)
            if (entries[e].flags & NFISAM_TRAJ_ALIGNED) sx.add(entries[e].ax), sy.add(entries[e].ay);
        abar_x = sx.value() / (double)aligned, abar_y = sy.value() / (double)aligned;
    }
    const int n_tiles = (n + 63) / 64;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(traj_error_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, Xt, x_rows, n, entries_dev, P, mode,
                       reflect != 0 ? 1 : 0, abar_x, abar_y, (double)(aligned > 0 ? aligned : 1), weights, out, iout, scratch);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(traj_entry_reduce_kernel, dim3((unsigned)((P + 1 + 255) / 256)), dim3(256), 0, s, scratch, n_tiles, P,
                           entry_sums);
        e = hipGetLastError();
    }
    return launch_status(e);
}

extern "C" int nfisam_sample_trajectory_rpe(const float* Xt, int x_rows, int n, const nfisam_traj_entry* entries,
                                            const nfisam_traj_entry* entries_dev, int P, const nfisam_traj_pair* pairs,
                                            const nfisam_traj_pair* pairs_dev, int n_pairs, int n_slots, double* out,
                                            nfisam_stream_t stream) {
    static_assert(sizeof(nfisam_traj_pair) == 16, "nfisam_traj_pair is 16 bytes");
    if (Xt == nullptr || entries == nullptr || entries_dev == nullptr || pairs == nullptr || pairs_dev == nullptr || out == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 1 || P < 1 || n_pairs < 1 || n_slots < 1 || n_slots > 65535) return NFISAM_ERR_ARG;
    if (check_entries(entries, P, x_rows) < 0) return NFISAM_ERR_ARG;
    for (int p = 0; p < n_pairs; ++p) {                            // `pairs` is the HOST copy: read here only
        const nfisam_traj_pair& Q = pairs[p];
        if (Q.i < 0 || Q.i >= P || Q.j < 0 || Q.j >= P || Q.slot < 0 || Q.slot >= n_slots) return NFISAM_ERR_ARG;
        if (entries[Q.i].col_th < 0 || entries[Q.j].col_th < 0) return NFISAM_ERR_ARG;       // a pair needs two headings
    }
    hipLaunchKernelGGL(traj_rpe_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)n_slots), dim3(256), 0, (hipStream_t)stream, Xt,
                       x_rows, n, entries_dev, P, pairs_dev, n_pairs, out);
    return launch_status(hipGetLastError());
}
