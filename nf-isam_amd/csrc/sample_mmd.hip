// sample_mmd.hip — the kernel sums of the two-sample maximum mean discrepancy, for many column blocks in one launch.
//
// The reference grades a posterior against a reference sample set with an RBF-kernel MMD (src/utils/Statistics.py:13-84,
// icra_paper/compute_mmd.py: one joint value per step plus the mean over the variables of the xy-marginal values): ~800 numpy
// calls per Plaza1 step, three dense Gram matrices each.  Here the two sets are column-major float32 device matrices (the
// layout of the tree walk's St) and a block is a list of (row of Xt, row of Yt) pairs; all blocks of a table are evaluated
// by one launch:
//     sums[b] = { sum_{i,i'} k_b(x_i, x_i'),  sum_{j,j'} k_b(y_j, y_j'),  sum_{i,j} k_b(x_i, y_j) }   (all ordered pairs),
//     k_b(u, v) = exp(-inv_two_sigma2_b * sum_e (scale_e * wrap_e(u_e - v_e))^2).
// The estimators (MMDb, MMDu2, the reference's `mmd`) are formed from the three sums on the host.
//
// Numerics: float32 points in; differences, squared distance, exp and every sum are float64 (the contract of
// sample_common.h).  Direct differences, never the Gram identity |x|^2 + |y|^2 - 2 x.y, which cancels at coordinates of
// 100 m; MMD^2 is a small difference of O(1) means, so float32 kernel values would cost three digits of it.
//
// Two launches, no float atomics.  (1) a 256-thread group owns one tile of pairs (sample_pairs.h) of one block and one of the
// three sums, 16 double accumulators of squared distance a lane, the i side from A and the j side from B through their own
// row tables; then 16 exp, the lane's sum in j order, wave_sum, the four waves in order, one store to partial[b][tile].  Sxx
// and Syy visit the upper triangle of tiles and count the off-diagonal ones twice (exact).  (2) one wave per (block, sum) adds
// the tile partials in an order that depends on (m, n) alone.  The block index is blockIdx.y and everything a block brings
// is wave-uniform.  Hence: two calls give the same bits, and a block's sums are the same bits alone or among hundreds,
// wherever it stands in the table.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

// tiles of the upper triangle (tj >= ti) of a T x T grid are numbered row by row; row ti starts at tri_off(ti, T)
__host__ __device__ __forceinline__ long long tri_off(long long ti, long long T) { return ti * T - ti * (ti - 1) / 2; }

__device__ __forceinline__ void tri_decode(long long t, int T, int* ti_out, int* tj_out) {
    const double s = 2.0 * T + 1.0;
    long long ti = (long long)((s - sqrt(fmax(s * s - 8.0 * (double)t, 0.0))) * 0.5);
    if (ti < 0) ti = 0;
    if (ti > T - 1) ti = T - 1;
    while (ti + 1 < T && tri_off(ti + 1, T) <= t) ++ti;
    while (ti > 0 && tri_off(ti, T) > t) --ti;
    *ti_out = (int)ti;
    *tj_out = (int)(ti + (t - tri_off(ti, T)));
}

template <bool WRAP, bool SCALE>
__device__ __forceinline__ void column_step(double (&acc)[JPL], double xi, const double* __restrict__ yrow, double sc) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        double diff = xi - yrow[jj];
        if (WRAP) diff = wrap_pi(diff);
        if (SCALE) diff *= sc;
        acc[jj] = fma(diff, diff, acc[jj]);
    }
}

// grid (tiles of Sxx | tiles of Syy | tiles of Sxy, blocks); 256 threads
__global__ void __launch_bounds__(256) mmd_tile_kernel(const nfisam_mmd_block* __restrict__ blocks, const float* __restrict__ Xt,
                                                       int x_rows, int m, const float* __restrict__ Yt, int y_rows, int n,
                                                       const int32_t* __restrict__ xcols, const int32_t* __restrict__ ycols,
                                                       int n_entries, const double* __restrict__ scale,
                                                       const uint8_t* __restrict__ wrap, int Tx, int Ty, long long tiles_total,
                                                       double* __restrict__ partial) {
    __shared__ double ys[CH][TILE];
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const long long t = blockIdx.x;
    const long long nxx = tri_off(Tx, Tx), nyy = tri_off(Ty, Ty);

    // which sum and which tile of it: blockIdx alone decides, so all of it is wave-uniform
    const float* __restrict__ A;
    const float* __restrict__ B;
    const int32_t* __restrict__ acols;
    const int32_t* __restrict__ bcols;
    int a_rows, b_rows, an, bn, ti, tj;
    double weight = 1.0;
    if (t < nxx) {
        tri_decode(t, Tx, &ti, &tj);
        A = B = Xt, acols = bcols = xcols, a_rows = b_rows = x_rows, an = bn = m;
        if (tj != ti) weight = 2.0;
    } else if (t < nxx + nyy) {
        tri_decode(t - nxx, Ty, &ti, &tj);
        A = B = Yt, acols = bcols = ycols, a_rows = b_rows = y_rows, an = bn = n;
        if (tj != ti) weight = 2.0;
    } else {
        const long long r = t - nxx - nyy;
        ti = (int)(r / Ty), tj = (int)(r % Ty);
        A = Xt, B = Yt, acols = xcols, bcols = ycols, a_rows = x_rows, b_rows = y_rows, an = m, bn = n;
    }

    const int col_off = blocks[b].col_off, d = blocks[b].d;
    const double inv = blocks[b].inv_two_sigma2;
    // a block whose entries leave the tables is never walked; a row outside its matrix is replaced by row 0: NaN either way
    bool bad = col_off < 0 || d < 1 || (long long)col_off + d > n_entries;
    const int d_walk = bad ? 0 : d;

    const int i = ti * TILE + lane;
    const size_t ic = (size_t)(i < an ? i : an - 1);
    const int jl = tj * TILE + lane;                                   // the j this thread stages
    const size_t jc = (size_t)(jl < bn ? jl : bn - 1);

    double acc[JPL];
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) acc[jj] = 0.0;

    for (int c0 = 0; c0 < d_walk; c0 += CH) {
        const int cnt = min(CH, d_walk - c0);
        __syncthreads();                                               // the previous chunk's tile has been read
#pragma unroll
        for (int k = 0; k < CH / 4; ++k) {                             // wave w stages columns w, w + 4, ...
            const int c = w + 4 * k;
            if (c < cnt) {
                int row = bcols[col_off + c0 + c];
                if (row < 0 || row >= b_rows) bad = true, row = 0;
                ys[c][lane] = (double)B[(size_t)row * bn + jc];
            }
        }
        float xa[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {                                 // the i side: one coalesced row read per column
            xa[c] = 0.0f;
            if (c < cnt) {
                int row = acols[col_off + c0 + c];
                if (row < 0 || row >= a_rows) bad = true, row = 0;
                xa[c] = A[(size_t)row * an + ic];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c < cnt) {
                const int e = col_off + c0 + c;
                const bool wr = wrap != nullptr && wrap[e] != 0;
                const double xi = (double)xa[c];
                const double* __restrict__ yrow = &ys[c][w * JPL];
                if (scale != nullptr) {
                    const double sc = scale[e];
                    if (wr) column_step<true, true>(acc, xi, yrow, sc);
                    else column_step<false, true>(acc, xi, yrow, sc);
                } else {
                    if (wr) column_step<true, false>(acc, xi, yrow, 1.0);
                    else column_step<false, false>(acc, xi, yrow, 1.0);
                }
            }
        }
    }

    double s = 0.0;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        const int j = tj * TILE + w * JPL + jj;
        const double k = exp(-inv * acc[jj]);
        s += (i < an && j < bn) ? k : 0.0;
    }
    s = wave_sum(s);
    // `bad` is uniform within a wave (it depends on the tables alone) but each wave has seen only the rows it staged
    __shared__ int bad_any[4];
    if (lane == 0) wsum[w] = s, bad_any[w] = bad ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = waves_in_order(wsum);
        const bool any = (bad_any[0] | bad_any[1] | bad_any[2] | bad_any[3]) != 0;
        partial[(size_t)b * (size_t)tiles_total + (size_t)t] = any ? (double)NAN : weight * tot;
    }
}

// grid (3, blocks), one wave: sums[b][which] = the tile partials of that sum; lane l adds tiles l, l + 64, ... in order, then
// the fixed tree -- an order that depends on the tile counts alone
__global__ void __launch_bounds__(64) mmd_sum_kernel(const double* __restrict__ partial, int Tx, int Ty, long long tiles_total,
                                                     double* __restrict__ sums) {
    const int which = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const long long nxx = tri_off(Tx, Tx), nyy = tri_off(Ty, Ty);
    const long long start = which == 0 ? 0 : which == 1 ? nxx : nxx + nyy;
    const long long cnt = which == 0 ? nxx : which == 1 ? nyy : (long long)Tx * Ty;
    const double* __restrict__ p = partial + (size_t)b * (size_t)tiles_total + (size_t)start;
    double s = 0.0;
    for (long long k = lane; k < cnt; k += 64) s += p[k];
    s = wave_sum(s);
    if (lane == 0) sums[(size_t)b * 3 + which] = s;
}

bool tile_counts(int m, int n, int* Tx, int* Ty, long long* total) {
    if (!tile_count(m, Tx) || !tile_count(n, Ty)) return false;
    *total = tri_off(*Tx, *Tx) + tri_off(*Ty, *Ty) + (long long)*Tx * *Ty;
    return *total <= 2147483647LL;                                 // the grid's first dimension (65536 tiles a side are past it)
}

}  // namespace

extern "C" size_t nfisam_sample_mmd_scratch_count(int m, int n, int n_blocks) {
    int Tx, Ty;
    long long total;
    if (n_blocks < 1 || !tile_counts(m, n, &Tx, &Ty, &total)) return 0;
    return (size_t)n_blocks * (size_t)total;                       // one partial per (block, tile)
}

extern "C" int nfisam_sample_mmd(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n,
                                 const nfisam_mmd_block* blocks, const nfisam_mmd_block* blocks_dev, int n_blocks,
                                 const int32_t* xcols, const int32_t* ycols, int n_entries, const double* scale,
                                 const uint8_t* wrap, double* sums, double* scratch, nfisam_stream_t stream) {
    if (Xt == nullptr || Yt == nullptr || blocks == nullptr || blocks_dev == nullptr || xcols == nullptr || ycols == nullptr || sums == nullptr ||
        scratch == nullptr)
        return NFISAM_ERR_ARG;
    if (x_rows < 1 || y_rows < 1 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535) return NFISAM_ERR_ARG;
    int Tx, Ty;
    long long total;
    if (!tile_counts(m, n, &Tx, &Ty, &total)) return NFISAM_ERR_ARG;
    if (!check_block_table(blocks, n_blocks)) return NFISAM_ERR_ARG;   // `blocks` is the HOST copy of the table
    hipStream_t s = (hipStream_t)stream;
    double* partial = scratch;
    hipLaunchKernelGGL(mmd_tile_kernel, dim3((unsigned)total, n_blocks), dim3(256), 0, s, blocks_dev, Xt, x_rows, m, Yt, y_rows, n,
                       xcols, ycols, n_entries, scale, wrap, Tx, Ty, total, partial);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mmd_sum_kernel, dim3(3, n_blocks), dim3(64), 0, s, partial, Tx, Ty, total, sums);
        e = hipGetLastError();
    }
    return launch_status(e);
}
