// sample_svgd.hip — moving posterior samples along the joint score: the Stein variational direction and the step that applies it.
//
// Every other unit over the sample matrix grades or describes the draw; this one moves it.  Stein variational gradient descent
// (Liu & Wang 2016) moves n particles along
//     phi(x_i) = 1/n sum_j [ k(x_j, x_i) grad log p(x_j) + grad_{x_j} k(x_j, x_i) ],
// the descent direction of the very statistic sample_ksd.hip reports: drawn towards p by the scores, kept apart by the kernel.
// Here the points are the column-major float32 matrix Xt[x_rows][n] (the tree walk's St), the scores the column-major float64
// matrix Gt[x_rows][n] that nfisam_factor_graph_score writes, and a block is a run of entries of the row list `cols`, as in
// sample_mmd.hip: its kernel sees the block's own columns only (the fixed point is still p, by integration by parts over those
// columns), so one table holds a block per variable or one block over all columns.  For block b, entry e, d_ij,e = x_i - x_j in
// row cols[e] (brought into [-pi, pi] as sign(d) wrap(|d|) where wrap[e] is set, so that d_ji = -d_ij to the bit):
//     k_b(i, j) = exp(-inv_two_sigma2 sum_e (scale_e d_ij,e)^2)
//     phi[e][i] = ( sum_j k_b(i, j) ( Gt[cols[e]][j] + 2 inv_two_sigma2 scale_e^2 d_ij,e ) ) / n
// An entry with scale_e = 0 leaves the kernel and still gets its sum_j k g / n.  The output is ENTRY-major, phi[n_entries][n]:
// blocks own disjoint entries, so two blocks never write the same address even if a row of Xt were named twice.
//
// Numerics: the contract of sample_common.h -- float32 points in; differences, products, exp and every sum float64; direct
// differences.
//
// Two launches, no float atomics.  (1) grid (T tiles of j, T tiles of i, blocks), a 256-thread group per tile of pairs
// (sample_pairs.h) and block.  Pass 1 walks the block's columns, points alone, to the 16 squared distances, then the 16 k, which
// stay in registers (zero for a pair outside the n x n square).  Pass 2 walks the columns again, points and scores of the j
// side staged, and forms per column the lane's sum over its 16 j in j order; the four waves' sums of a chunk are parked in LDS
// and combined in wave order, one store to partial[tj][e][i].  The block width has no limit: nothing is kept per column
// beyond the chunk.  (2) phi[e][i] = the partials of (e, i) in tile order, divided by n.  The split of the j range depends on
// n alone.  Hence: two calls give the same bits, a block's rows are the same bits alone or among hundreds, wherever it stands
// in the table.  A pair's two terms are mirror images to the bit (k_ij = k_ji, d_ji = -d_ij) and enter the sums as rounded
// products: swapping the two points of a two-point set swaps their phi rows bit for bit (among more points the terms are the
// same bits and only the order of the sum differs).
// LDS: 2 x 8 KiB staged tiles + 32 KiB of wave sums = 48 KiB a group, three groups a CU; the partials take
// T x n_entries x 64 T doubles (nfisam_sample_svgd_scratch_count).
//
// THE STEP (nfisam_sample_step) applies the AdaGrad-with-decay rule of the original SVGD code to every (entry, point), float64:
//     hist = first ? phi^2 : alpha hist + (1 - alpha) phi^2
//     y    = (double)Xt[cols[e]][i] + eps[e] phi / (sqrt(hist) + fudge)
//     Xt[cols[e]][i] = (float)(wrap[e] ? wrap_pi(y) : y)
// and writes the float32 matrix in place.  The points stay float32, which is what every evaluator here reads: A STEP SMALLER
// THAN THE FLOAT32 SPACING OF A COORDINATE IS LOST -- 7.6e-6 at 100 m.  A wrapped value that rounds to +-float32(pi), which lies
// outside [-pi, pi), becomes the float32 just inside -pi (-3.1415925): the same angle to 2.4e-7.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

template <bool WRAP>
__device__ __forceinline__ void distance_step(double (&acc)[JPL], double xi, const double* __restrict__ xrow, double sc) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        double d = xi - xrow[jj];
        if (WRAP) d = signed_wrap(d);
        d *= sc;
        acc[jj] = fma(d, d, acc[jj]);
    }
}

template <bool WRAP>
__device__ __forceinline__ double direction_step(const double (&k)[JPL], double xi, const double* __restrict__ xrow,
                                                 const double* __restrict__ grow, double coef) {
    double s = 0.0;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {                                  // the lane's 16 j, in j order
        double d = xi - xrow[jj];
        if (WRAP) d = signed_wrap(d);
        // a ROUNDED product, then a plain sum: the two terms of a pair of points add to the same bits in either order, which a
        // fused multiply-add into the running sum would not give (the swap promise of the header comment).  The unit is built
        // with -ffp-contract=fast, which fuses across a contract pragma: the empty statement makes the product opaque instead.
        double t = k[jj] * fma(coef, d, grow[jj]);
        asm("" : "+v"(t));
        s = s + t;
    }
    return s;
}

// grid (T tiles of j, T tiles of i, blocks); 256 threads.  Three waves a SIMD are asked for (left alone the compiler takes 170 VGPRs and
// fits two; asked, it takes 134 and spills nothing), which is also what the 48 KiB of LDS allow: three groups a CU
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) svgd_tile_kernel(const nfisam_mmd_block* __restrict__ blocks, const float* __restrict__ Xt,
                                                        int x_rows, int n, const double* __restrict__ Gt,
                                                        const int32_t* __restrict__ cols, int n_entries,
                                                        const double* __restrict__ scale, const uint8_t* __restrict__ wrap,
                                                        double* __restrict__ partial) {
    __shared__ double xs[CH][TILE];
    __shared__ double gs[CH][TILE];
    __shared__ double wsum[CH][4][TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tj = blockIdx.x, ti = blockIdx.y, b = blockIdx.z;
    const size_t i_pad = (size_t)gridDim.y * TILE;                     // the partials' row length: T tiles of 64 i

    const int col_off = blocks[b].col_off, d = blocks[b].d;
    const double inv = blocks[b].inv_two_sigma2;
    // a block whose entries leave the table is never walked here (the second launch writes NaN where its entries lie inside)
    if (col_off < 0 || d < 1 || (long long)col_off + d > n_entries) return;
    bool bad = false;                                                  // a row outside the matrix: read as row 0, NaN out

    const int i = ti * TILE + lane;
    const size_t ic = (size_t)(i < n ? i : n - 1);
    const int jl = tj * TILE + lane;                                   // the j this thread stages
    const size_t jc = (size_t)(jl < n ? jl : n - 1);

    // ---- pass 1: the 16 squared distances of the lane's pairs, then the 16 kernel values ----------------------------------
    double k[JPL];
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) k[jj] = 0.0;
    for (int c0 = 0; c0 < d; c0 += CH) {
        const int cnt = min(CH, d - c0);
        __syncthreads();                                               // the previous chunk's tile has been read
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {                             // wave w stages columns w, w + 4, ...
            const int c = w + 4 * q;
            if (c < cnt) {
                int row = cols[col_off + c0 + c];
                if (row < 0 || row >= x_rows) row = 0;
                xs[c][lane] = (double)Xt[(size_t)row * n + jc];
            }
        }
        float xa[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {                                 // the i side: one coalesced row read per column
            xa[c] = 0.0f;
            if (c < cnt) {
                int row = cols[col_off + c0 + c];
                if (row < 0 || row >= x_rows) bad = true, row = 0;     // (every thread sees every row of the block)
                xa[c] = Xt[(size_t)row * n + ic];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c < cnt) {
                const int e = col_off + c0 + c;
                const double sc = scale != nullptr ? scale[e] : 1.0;
                if (wrap != nullptr && wrap[e] != 0) distance_step<true>(k, (double)xa[c], &xs[c][w * JPL], sc);
                else distance_step<false>(k, (double)xa[c], &xs[c][w * JPL], sc);
            }
        }
    }
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        const int j = tj * TILE + w * JPL + jj;
        k[jj] = (i < n && j < n) ? exp(-inv * k[jj]) : 0.0;
    }

    // ---- pass 2: per column, sum_j k (g_j + coef d_ij) over the tile's j ---------------------------------------------------------
    for (int c0 = 0; c0 < d; c0 += CH) {
        const int cnt = min(CH, d - c0);
        __syncthreads();                                               // the previous chunk's tiles and wave sums have been read
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            const int c = w + 4 * q;
            if (c < cnt) {
                int row = cols[col_off + c0 + c];
                if (row < 0 || row >= x_rows) row = 0;
                xs[c][lane] = (double)Xt[(size_t)row * n + jc];
                gs[c][lane] = Gt[(size_t)row * n + jc];
            }
        }
        float xa[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            xa[c] = 0.0f;
            if (c < cnt) {
                int row = cols[col_off + c0 + c];
                if (row < 0 || row >= x_rows) row = 0;
                xa[c] = Xt[(size_t)row * n + ic];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c < cnt) {
                const int e = col_off + c0 + c;
                const double sc = scale != nullptr ? scale[e] : 1.0;
                const double coef = 2.0 * inv * (sc * sc);
                double s;
                if (wrap != nullptr && wrap[e] != 0) s = direction_step<true>(k, (double)xa[c], &xs[c][w * JPL], &gs[c][w * JPL], coef);
                else s = direction_step<false>(k, (double)xa[c], &xs[c][w * JPL], &gs[c][w * JPL], coef);
                wsum[c][w][lane] = s;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {                             // wave w combines columns w, w + 4, ...: the waves in order
            const int c = w + 4 * q;
            if (c < cnt) {
                const double p4[4] = {wsum[c][0][lane], wsum[c][1][lane], wsum[c][2][lane], wsum[c][3][lane]};
                const size_t e = (size_t)(col_off + c0 + c);
                partial[((size_t)tj * (size_t)n_entries + e) * i_pad + (size_t)i] = bad ? (double)NAN : waves_in_order(p4);
            }
        }
    }
}

// grid (T tiles of i, blocks, slices of the block's columns); 256 threads: wave w of slice z takes the block's columns
// 4 z + w, + 4 slices, ...; phi[e][i] = the partials of (e, i) in tile order, over n
__global__ void __launch_bounds__(256) svgd_sum_kernel(const nfisam_mmd_block* __restrict__ blocks, const double* __restrict__ partial,
                                                       int T, int n, int n_entries, double* __restrict__ phi) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * TILE + lane, b = blockIdx.y;
    if (i >= n) return;
    const long long col_off = blocks[b].col_off, d = blocks[b].d;
    const bool bad = col_off < 0 || d < 1 || col_off + d > n_entries;
    const size_t i_pad = (size_t)T * TILE;
    for (long long c = 4 * (long long)blockIdx.z + w; c < d; c += 4 * (long long)gridDim.z) {
        const long long e = col_off + c;
        if (e < 0 || e >= n_entries) continue;                         // (a bad block: NaN where its entries lie inside)
        double s = 0.0;
        if (bad) s = (double)NAN;
        else
            for (int t = 0; t < T; ++t) s += partial[((size_t)t * (size_t)n_entries + (size_t)e) * i_pad + (size_t)i];
        phi[(size_t)e * n + i] = s / (double)n;
    }
}

// grid (tiles of 256 points, entries); 256 threads
__global__ void __launch_bounds__(256) svgd_step_kernel(float* __restrict__ Xt, int x_rows, int n, const int32_t* __restrict__ cols,
                                                        const uint8_t* __restrict__ wrap, const double* __restrict__ phi,
                                                        double* __restrict__ hist, const double* __restrict__ eps, double alpha,
                                                        double fudge, int first) {
    const int i = blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
    if (i >= n) return;
    const size_t at = (size_t)e * n + i;
    const int row = cols[e];
    if (row < 0 || row >= x_rows) {                                    // no such row: nothing moves, the state says so
        hist[at] = (double)NAN;
        return;
    }
    const double p = phi[at];
    const double h = first ? p * p : alpha * hist[at] + (1.0 - alpha) * (p * p);
    hist[at] = h;
    const size_t xi = (size_t)row * n + i;
    const double y = (double)Xt[xi] + eps[e] * p / (sqrt(h) + fudge);
    float f = (float)y;
    if (wrap != nullptr && wrap[e] != 0) {
        f = (float)wrap_pi(y);
        if (!((double)f < PI && (double)f >= -PI)) f = -3.1415925f;   // +-float32(pi) lies outside: the float32 just inside -pi
        if (isnan(y)) f = (float)y;
    }
    Xt[xi] = f;
}

}  // namespace

extern "C" size_t nfisam_sample_svgd_scratch_count(int n, int n_blocks, int n_entries) {
    int T;
    if (n_blocks < 1 || n_blocks > 65535 || n_entries < 1 || !tile_count(n, &T)) return 0;
    return (size_t)T * (size_t)n_entries * ((size_t)T * TILE);         // one partial per (tile of j, entry, i)
}

extern "C" int nfisam_sample_svgd(const float* Xt, int x_rows, int n, const double* Gt, const nfisam_mmd_block* blocks,
                                  const nfisam_mmd_block* blocks_dev, int n_blocks, const int32_t* cols, int n_entries,
                                  const double* scale, const uint8_t* wrap, double* phi, double* scratch, nfisam_stream_t stream) {
    if (Xt == nullptr || Gt == nullptr || blocks == nullptr || blocks_dev == nullptr || cols == nullptr || phi == nullptr ||
        scratch == nullptr)
        return NFISAM_ERR_ARG;
    int T;
    if (x_rows < 1 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535 || !tile_count(n, &T)) return NFISAM_ERR_ARG;
    if (!check_block_table(blocks, n_blocks)) return NFISAM_ERR_ARG;   // `blocks` is the HOST copy of the table
    long long max_d = 1;
    std::vector<std::pair<long long, long long>> runs((size_t)n_blocks);
    for (int b = 0; b < n_blocks; ++b) {
        max_d = std::max<long long>(max_d, blocks[b].d);
        runs[(size_t)b] = {blocks[b].col_off, (long long)blocks[b].col_off + blocks[b].d};
    }
    std::sort(runs.begin(), runs.end());                               // an entry has one direction: no two blocks share one
    for (int b = 1; b < n_blocks; ++b)
        if (runs[(size_t)b].first < runs[(size_t)b - 1].second) return NFISAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(svgd_tile_kernel, dim3(T, T, n_blocks), dim3(256), 0, s, blocks_dev, Xt, x_rows, n, Gt, cols, n_entries, scale,
                       wrap, scratch);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const unsigned slices = (unsigned)std::min<long long>((max_d + 3) / 4, 65535);
        hipLaunchKernelGGL(svgd_sum_kernel, dim3(T, n_blocks, slices), dim3(256), 0, s, blocks_dev, scratch, T, n, n_entries, phi);
        e = hipGetLastError();
    }
    return launch_status(e);
}

extern "C" int nfisam_sample_step(float* Xt, int x_rows, int n, const int32_t* cols, int n_entries, const uint8_t* wrap,
                                  const double* phi, double* hist, const double* eps, double alpha, double fudge, int first,
                                  nfisam_stream_t stream) {
    if (Xt == nullptr || cols == nullptr || phi == nullptr || hist == nullptr || eps == nullptr) return NFISAM_ERR_ARG;
    if (x_rows < 1 || n < 1 || n_entries < 1 || n_entries > 65535) return NFISAM_ERR_ARG;     // the grid's second dimension
    if (!(alpha >= 0.0 && alpha < 1.0) || !(fudge > 0.0) || !isfinite(fudge)) return NFISAM_ERR_ARG;
    hipLaunchKernelGGL(svgd_step_kernel, dim3((unsigned)(((long long)n + 255) / 256), n_entries), dim3(256), 0, (hipStream_t)stream, Xt,
                       x_rows, n, cols, wrap, phi, hist, eps, alpha, fudge, first);
    return launch_status(hipGetLastError());
}
