// sample_density.hip — a sample set's marginal density AT POINTS THE CALLER CHOOSES: the Gaussian kernel density estimate of
// many column blocks at many queries, in logs.  What a marginal's curve on a grid, a map over the plane, the negative log
// predictive density at the ground truth and the level of the smallest highest-density region that holds it are formed
// from (utils/Statistics.py: sample_density_t, hpd_level; the reference runs scipy.stats.gaussian_kde per coordinate on the
// host, example/slam/*/kde_plot_grid.py).  sample_modes.hip evaluates the same kind of estimate at its own converged starts
// only, under an isotropic bandwidth on standardised columns; here the bandwidth is a full matrix H per block.
//
// Qt [q_rows][m] holds the queries and Xt [x_rows][n] the samples (COLUMN-major float32 device matrices, the layout of
// sample_common.h; they may be one matrix); entry e pairs row qcols[e] of Qt with row xcols[e] of Xt and a block is a run of
// 1..6 entries with a lower-triangular whitening matrix W (W H W' = I) and the constant log_norm = sum_r log W_rr - d/2 log 2 pi.
// For block b, query i, sample j
//     diff_c = (double)x_jc - (double)q_ic               (wrapped into [-pi, pi) by wrap_pi_near where wrap[e] is set)
//     u_r    = sum_{c <= r} W_rc diff_c                  (c ascending, every step an fma)
//     e_ij   = -1/2 sum_r u_r^2 + log_w[j]               (r ascending, fma; log_w NULL: 0)
//     log_dens[b][i] = ((log_norm + M_i) + log(sum_j exp(e_ij - M_i))) - log W_tot,      M_i = max_j e_ij.
//
// Numerics: float32 points in; every difference, product, transcendental and sum is float64 (the contract of
// sample_common.h).  The shift by the max makes the log usable in the tails: a query 1e4 bandwidths from every sample has
// e about -5e7, whose exp is 0, but its largest term is exp(0) = 1 and the log is finite.  Two sweeps over the samples -- the
// max, then the sum -- cost ONE float64 exp per pair; the online form that rescales its running sum costs up to two.
//
// density_kernel, grid (ceil(m / 64), blocks), 256 threads: a group owns 64 queries, one per lane, the same 64 in each of the
// four waves.  A sweep walks the n samples in chunks of 128 staged as doubles in LDS ([7][128]: the block's columns and
// log_w), wave w taking the chunk's j = 32 w .. 32 w + 31 by broadcast reads; a set of n <= 128 is staged once for both
// sweeps.  Sweep 1: a thread's running max; the four meet in LDS (a max is exact in any order; a NaN is kept, not swallowed).
// Sweep 2: a thread adds exp(e - M) with its j ascending, then the four waves by waves_in_order.  That order depends on n
// alone: two calls give the same bits, a block's rows are the same bits alone, repeated, or anywhere in a table, and a
// query's result depends neither on m nor on its tile.  No float atomics.  Everything a group brings is decided by blockIdx
// alone (wave-uniform).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

constexpr int MAX_D = NFISAM_DENSITY_MAX_D;
constexpr int NW = MAX_D * (MAX_D + 1) / 2;   // packed lower triangle
constexpr int QPG = 64;           // queries per group: one per lane, the same 64 in each of the four waves
constexpr int JT = 128;           // samples j per staged chunk
constexpr int JPW = JT / 4;       // ... of which a wave takes 32
constexpr int ROWS = MAX_D + 1;   // staged rows: the columns and log_w
static_assert(QPG == TILE, "tile_count counts the groups of queries");
static_assert(NW == 21 && sizeof(nfisam_density_block) == 16 + 8 * NW, "nfisam_density_block is 184 bytes");

// what a block brings, the same in every thread of its groups
struct BlockHead {
    int col_off, d;
    double log_norm;
    bool bad;                      // entries outside the lists, a row outside its matrix, d outside 1..6: never walked
};

__device__ __forceinline__ BlockHead block_head(const nfisam_density_block* __restrict__ blocks, int b, const int32_t* __restrict__ qcols,
                                                const int32_t* __restrict__ xcols, int n_entries, int q_rows, int x_rows) {
    BlockHead h;
    h.col_off = blocks[b].col_off, h.d = blocks[b].d, h.log_norm = blocks[b].log_norm;
    h.bad = h.d < 1 || h.d > MAX_D || h.col_off < 0 || (long long)h.col_off + h.d > n_entries;
    if (!h.bad)
        for (int c = 0; c < h.d; ++c) {
            const int rq = qcols[h.col_off + c], rx = xcols[h.col_off + c];
            if (rq < 0 || rq >= q_rows || rx < 0 || rx >= x_rows) h.bad = true;
        }
    return h;
}

// the larger of two energies; a NaN is kept whichever side it stands on
__device__ __forceinline__ double nan_max(double a, double e) { return (e > a || e != e) ? e : a; }

// both sweeps of the group's 64 queries, for a block of d <= DM columns (DM picks the unrolled width; rows and columns >= d
// of the register arrays are never touched)
template <int DM>
__device__ __forceinline__ void walk(const BlockHead h, const float* __restrict__ Qt, int m, const float* __restrict__ Xt, int n,
                                     int exclude_self, const int* rq_s, const int* rx_s, const double* W_s,
                                     const uint8_t* __restrict__ wrap, const double* __restrict__ log_w, double log_w_sum,
                                     double (*xs)[JT], double (*part)[4], double* __restrict__ log_dens, double* __restrict__ dens) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tid = threadIdx.x;
    const int d = h.d, b = blockIdx.y;
    const int i = blockIdx.x * QPG + lane;

    // W and the query come from LDS / global into vector registers: the scalar file is left to the loop
    double W[DM * (DM + 1) / 2], q[DM];
    unsigned wrap_mask = 0;
#pragma unroll
    for (int r = 0; r < DM; ++r) {
        q[r] = 0.0;
#pragma unroll
        for (int c = 0; c <= r; ++c) W[r * (r + 1) / 2 + c] = r < d ? W_s[r * (r + 1) / 2 + c] : 0.0;
        if (r < d) {
            if (wrap != nullptr && wrap[h.col_off + r] != 0) wrap_mask |= 1u << r;
            if (i < m) q[r] = (double)Qt[(size_t)rq_s[r] * (size_t)m + (size_t)i];
        }
    }
    const bool skip_self = exclude_self != 0;
    const bool stage_once = n <= JT;                               // one chunk: it stays in LDS for both sweeps

    double M = -(double)INFINITY, s = 0.0;
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int j0 = 0; j0 < n; j0 += JT) {
            if (!stage_once || sweep == 0) {
                __syncthreads();                                   // the previous chunk has been read
                if (tid < JT) {
                    const int j = j0 + tid;
                    const bool in = j < n;
                    for (int c = 0; c < d; ++c)
                        xs[c][tid] = in ? (double)Xt[(size_t)rx_s[c] * (size_t)n + (size_t)j] : 0.0;
                    xs[MAX_D][tid] = in ? (log_w != nullptr ? log_w[j] : 0.0) : -(double)INFINITY;
                }
                __syncthreads();
            }
            const int cnt = min(JT, n - j0);
            const int jb = w * JPW, je = min(jb + JPW, cnt);
            for (int jl = jb; jl < je; ++jl) {
                if (skip_self && j0 + jl == i) continue;           // the leave-one-out density
                double diff[DM], qq = 0.0;
#pragma unroll
                for (int c = 0; c < DM; ++c) {
                    diff[c] = 0.0;
                    if (c < d) {
                        double t = xs[c][jl] - q[c];
                        if ((wrap_mask >> c) & 1u) t = wrap_pi_near(t);
                        diff[c] = t;
                    }
                }
#pragma unroll
                for (int r = 0; r < DM; ++r)
                    if (r < d) {
                        double u = 0.0;
#pragma unroll
                        for (int c = 0; c <= r; ++c) u = fma(W[r * (r + 1) / 2 + c], diff[c], u);
                        qq = fma(u, u, qq);
                    }
                const double e = fma(-0.5, qq, xs[MAX_D][jl]);
                if (sweep == 0) M = nan_max(M, e);
                else s += exp(e - M);
            }
        }
        if (sweep == 0) {                                          // the four running maxima meet: every wave takes the same M
            part[lane][w] = M;
            __syncthreads();
            M = nan_max(nan_max(nan_max(part[lane][0], part[lane][1]), part[lane][2]), part[lane][3]);
            __syncthreads();                                       // (read before sweep 2's sums are parked there)
        }
    }
    part[lane][w] = s;
    __syncthreads();
    if (w != 0 || i >= m) return;
    const double S = waves_in_order(part[lane]);
    double ld;
    if (M != M) {
        ld = (double)NAN;                                          // a NaN coordinate or weight
    } else if (M == -(double)INFINITY) {
        ld = -(double)INFINITY;                                    // nothing contributes: no other sample, or zero weights only
    } else {
        double log_total;
        if (log_w == nullptr) log_total = log((double)(n - (skip_self ? 1 : 0)));
        else if (!skip_self) log_total = log_w_sum;
        else log_total = log(exp(log_w_sum) - exp(log_w[i]));      // (m == n: i is a sample)
        ld = ((h.log_norm + M) + log(S)) - log_total;
    }
    log_dens[(size_t)b * (size_t)m + (size_t)i] = ld;
    if (dens != nullptr) dens[(size_t)b * (size_t)m + (size_t)i] = exp(ld);
}

// grid (ceil(m / 64), n_blocks); 256 threads
__global__ void __launch_bounds__(256) density_kernel(const nfisam_density_block* __restrict__ blocks, const float* __restrict__ Qt,
                                                      int q_rows, int m, const float* __restrict__ Xt, int x_rows, int n,
                                                      int exclude_self, const int32_t* __restrict__ qcols,
                                                      const int32_t* __restrict__ xcols, int n_entries,
                                                      const uint8_t* __restrict__ wrap, const double* __restrict__ log_w,
                                                      double log_w_sum, double* __restrict__ log_dens, double* __restrict__ dens) {
    __shared__ double xs[ROWS][JT];                                // 7 KiB: the staged chunk
    __shared__ double part[QPG][4];                                // 2 KiB: the waves' maxima, then their sums
    __shared__ double W_s[NW];
    __shared__ int rq_s[MAX_D], rx_s[MAX_D];
    const int b = blockIdx.y;
    const BlockHead h = block_head(blocks, b, qcols, xcols, n_entries, q_rows, x_rows);
    if (h.bad) {                                                   // (the whole group: no barrier is left waiting)
        const int i = blockIdx.x * QPG + (int)threadIdx.x;
        if (threadIdx.x < QPG && i < m) {
            log_dens[(size_t)b * (size_t)m + (size_t)i] = (double)NAN;
            if (dens != nullptr) dens[(size_t)b * (size_t)m + (size_t)i] = (double)NAN;
        }
        return;
    }
    if (threadIdx.x < NW) W_s[threadIdx.x] = blocks[b].whiten[threadIdx.x];
    if (threadIdx.x < MAX_D) {
        const bool in = (int)threadIdx.x < h.d;
        rq_s[threadIdx.x] = in ? qcols[h.col_off + threadIdx.x] : 0;
        rx_s[threadIdx.x] = in ? xcols[h.col_off + threadIdx.x] : 0;
    }
    __syncthreads();
    if (h.d <= 2) walk<2>(h, Qt, m, Xt, n, exclude_self, rq_s, rx_s, W_s, wrap, log_w, log_w_sum, xs, part, log_dens, dens);
    else if (h.d <= 3) walk<3>(h, Qt, m, Xt, n, exclude_self, rq_s, rx_s, W_s, wrap, log_w, log_w_sum, xs, part, log_dens, dens);
    else walk<MAX_D>(h, Qt, m, Xt, n, exclude_self, rq_s, rx_s, W_s, wrap, log_w, log_w_sum, xs, part, log_dens, dens);
}

// the HOST copy of the table: widths, and a finite log_norm and whitening triangle with a positive diagonal
bool table_ok(const nfisam_density_block* blocks, int n_blocks) {
    for (int b = 0; b < n_blocks; ++b) {
        const int d = blocks[b].d;
        if (d < 1 || d > MAX_D || !isfinite(blocks[b].log_norm)) return false;
        for (int r = 0; r < d; ++r)
            for (int c = 0; c <= r; ++c) {
                const double v = blocks[b].whiten[r * (r + 1) / 2 + c];
                if (!isfinite(v) || (c == r && !(v > 0.0))) return false;
            }
    }
    return true;
}

}  // namespace

extern "C" int nfisam_sample_density(const float* Qt, int q_rows, int m, const float* Xt, int x_rows, int n, int exclude_self,
                                     const nfisam_density_block* blocks, const nfisam_density_block* blocks_dev, int n_blocks,
                                     const int32_t* qcols, const int32_t* xcols, int n_entries, const uint8_t* wrap,
                                     const double* log_w, double log_w_sum, double* log_dens, double* dens, nfisam_stream_t stream) {
    if (Qt == nullptr || Xt == nullptr || blocks == nullptr || blocks_dev == nullptr || qcols == nullptr || xcols == nullptr ||
        log_dens == nullptr)
        return NFISAM_ERR_ARG;
    if (q_rows < 1 || x_rows < 1 || n < 1 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535) return NFISAM_ERR_ARG;
    int Tq;
    if (!tile_count(m, &Tq)) return NFISAM_ERR_ARG;
    if (exclude_self != 0 && m != n) return NFISAM_ERR_ARG;
    if (log_w != nullptr && !isfinite(log_w_sum)) return NFISAM_ERR_ARG;
    if (!table_ok(blocks, n_blocks)) return NFISAM_ERR_ARG;
    hipLaunchKernelGGL(density_kernel, dim3((unsigned)Tq, (unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, blocks_dev, Qt, q_rows,
                       m, Xt, x_rows, n, exclude_self, qcols, xcols, n_entries, wrap, log_w, log_w_sum, log_dens, dens);
    return launch_status(hipGetLastError());
}
