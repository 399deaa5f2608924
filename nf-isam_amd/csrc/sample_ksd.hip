// sample_ksd.hip — the pairwise sums of the Gaussian kernel Stein discrepancy.
//
// The reference's Gaussian_kernel_stein_discrepancy (src/utils/Statistics.py:216-245) grades n samples against the factor
// graph itself, through the score s_i = grad_x log p(x_i, Z): a Python double loop over the pairs with D x D matrix products
// inside.  Here the points are the column-major float32 matrix Xt[D][n] (the tree walk's St), the scores the column-major
// float64 matrix Gt[D][n] that nfisam_factor_graph_score writes, and the kernel precision is diagonal, P = diag(p), p_c >= 0.
// With d = x_i - x_j (brought into [-pi, pi] for columns flagged in `wrap`):
//     k_ij = exp(-1/2 sum_c p_c d_c^2)
//     h_ij = k_ij [ s_i.s_j + sum_c (s_ic - s_jc) p_c d_c - sum_c p_c^2 d_c^2 + sum_c p_c ]
// which is the reference's (p1 + p2 + p3 + p4) KXX[i, j] for a diagonal P.  Outputs: row[i] = sum_j h_ij over ALL j,
// diag[i] = h_ii = |s_i|^2 + sum_c p_c, and on request the matrix H[n][n]; the U- and V-statistics are formed on the host.
//
// Numerics: the contract of sample_common.h -- float32 points in; differences, products, exp and every sum float64.  Direct
// differences, never the Gram identity.  A wrapped difference is sign(d) wrap(|d|), so d_ji = -d_ij to the bit and H is
// symmetric to the bit.
//
// Two launches, no float atomics.  (1) the FULL T x T grid of tiles of pairs (sample_pairs.h; h is symmetric, but the
// transposed row contributions of an upper-triangle walk would need a second fixed-order pass).  Four accumulators per pair
// (sum p d^2, s.s, sum (s_i - s_j) p d, sum p^2 d^2: 64 doubles a lane), points AND scores on both sides, an entry being its
// own row: no table.  Then 16 exp, the lane's sum in j order, the four waves in order, one store to partial[tj][i].
// (2) row[i] = the partials of i in tile order.  Hence: two calls give the same bits, and `row` is the same bits with and
// without H.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

template <bool WRAP>
__device__ __forceinline__ void column_step(double (&q)[JPL], double (&ss)[JPL], double (&sd)[JPL], double (&pp)[JPL], double xi,
                                            double si, double pc, const double* __restrict__ xrow,
                                            const double* __restrict__ srow) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        double d = xi - xrow[jj];
        if (WRAP) d = signed_wrap(d);
        const double sj = srow[jj];
        const double pd = pc * d;
        q[jj] = fma(pd, d, q[jj]);
        ss[jj] = fma(si, sj, ss[jj]);
        sd[jj] = fma(si - sj, pd, sd[jj]);
        pp[jj] = fma(pd, pd, pp[jj]);
    }
}

// grid (T tiles of j, T tiles of i); 256 threads
__global__ void __launch_bounds__(256) ksd_tile_kernel(const float* __restrict__ Xt, const double* __restrict__ Gt, int D, int n,
                                                       const double* __restrict__ prec, const uint8_t* __restrict__ wrap,
                                                       double* __restrict__ partial, double* __restrict__ diag,
                                                       double* __restrict__ H) {
    __shared__ double xs[CH][TILE];
    __shared__ double gs[CH][TILE];
    __shared__ double wsum[4][TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tj = blockIdx.x, ti = blockIdx.y;
    const int i = ti * TILE + lane;
    const size_t ic = (size_t)(i < n ? i : n - 1);
    const int jl = tj * TILE + lane;                                   // the j this thread stages
    const size_t jc = (size_t)(jl < n ? jl : n - 1);

    double q[JPL], ss[JPL], sd[JPL], pp[JPL];
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) q[jj] = ss[jj] = sd[jj] = pp[jj] = 0.0;
    double sum_p = 0.0;                                                // sum_c p_c, in column order (wave-uniform)

    for (int c0 = 0; c0 < D; c0 += CH) {
        const int cnt = min(CH, D - c0);
        __syncthreads();                                               // the previous chunk's tiles have been read
#pragma unroll
        for (int k = 0; k < CH / 4; ++k) {                             // wave w stages columns w, w + 4, ...
            const int c = w + 4 * k;
            if (c < cnt) {
                xs[c][lane] = (double)Xt[(size_t)(c0 + c) * n + jc];
                gs[c][lane] = Gt[(size_t)(c0 + c) * n + jc];
            }
        }
        float xa[CH];
        double ga[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {                                 // the i side: one coalesced row read per column
            xa[c] = 0.0f, ga[c] = 0.0;
            if (c < cnt) {
                xa[c] = Xt[(size_t)(c0 + c) * n + ic];
                ga[c] = Gt[(size_t)(c0 + c) * n + ic];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c < cnt) {
                const double pc = prec[c0 + c];
                sum_p += pc;
                const bool wr = wrap != nullptr && wrap[c0 + c] != 0;
                if (wr) column_step<true>(q, ss, sd, pp, (double)xa[c], ga[c], pc, &xs[c][w * JPL], &gs[c][w * JPL]);
                else column_step<false>(q, ss, sd, pp, (double)xa[c], ga[c], pc, &xs[c][w * JPL], &gs[c][w * JPL]);
            }
        }
    }

    double s = 0.0;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        const int j = tj * TILE + w * JPL + jj;
        const double h = exp(-0.5 * q[jj]) * (((ss[jj] + sd[jj]) - pp[jj]) + sum_p);
        const bool in = i < n && j < n;
        s += in ? h : 0.0;
        if (in && H != nullptr) H[(size_t)i * n + j] = h;
        if (in && i == j) diag[i] = h;                                 // k_ii = 1, d = 0: |s_i|^2 + sum_p
    }
    wsum[w][lane] = s;
    __syncthreads();
    if (w == 0) {
        const double p4[4] = {wsum[0][lane], wsum[1][lane], wsum[2][lane], wsum[3][lane]};
        partial[(size_t)tj * ((size_t)gridDim.y * TILE) + (size_t)i] = waves_in_order(p4);
    }
}

// grid (T), one wave: row[i] = the partials of i in tile order
__global__ void __launch_bounds__(64) ksd_row_kernel(const double* __restrict__ partial, int T, int n, double* __restrict__ row) {
    const int i = blockIdx.x * TILE + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += partial[(size_t)t * ((size_t)T * TILE) + (size_t)i];
    row[i] = s;
}

}  // namespace

extern "C" size_t nfisam_sample_ksd_scratch_count(int n) {
    int T;
    if (!tile_count(n, &T)) return 0;
    return (size_t)T * (size_t)T * TILE;                               // one partial per (tile of j, i)
}

extern "C" int nfisam_sample_ksd(const float* Xt, const double* Gt, int rows, int n, const double* precision, const uint8_t* wrap,
                                 double* row, double* diag, double* H, double* scratch, nfisam_stream_t stream) {
    if (Xt == nullptr || Gt == nullptr || precision == nullptr || row == nullptr || diag == nullptr || scratch == nullptr)
        return NFISAM_ERR_ARG;
    int T;
    if (rows < 1 || !tile_count(n, &T)) return NFISAM_ERR_ARG;
    if (H != nullptr && n > NFISAM_KSD_MATRIX_MAX_N) return NFISAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ksd_tile_kernel, dim3(T, T), dim3(256), 0, s, Xt, Gt, rows, n, precision, wrap, scratch, diag, H);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ksd_row_kernel, dim3(T), dim3(64), 0, s, scratch, T, n, row);
        e = hipGetLastError();
    }
    return launch_status(e);
}
