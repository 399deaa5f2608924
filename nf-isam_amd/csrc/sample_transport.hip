// sample_transport.hip — the sliced Wasserstein distance between two sample sets, every (block, direction) slice in one launch.
//
// What the MMD cannot say: how far, in the variables' own units, the posterior must be moved to become the reference set.  A
// slice projects both sets onto one direction, sorts the two lists of keys and integrates the difference of the two quantile
// functions; a block's distance is the mean (or the maximum) of its slices, formed on the host.  With a basis vector as the
// direction a slice is the exact 1-D Wasserstein distance of that entry's marginal.  Nothing of this is in the reference
// (its src/utils/Statistics.py stops at MMD, RMSE and KSD).
//
//     key(x; b, j) = sum_e dir[b][j][e] * scale[e] * f_kind[e]((double)x_e)          (ascending e; f: the value, cos or sin)
//     out[b][j]    = W_p^p = int_0^1 |F_X^-1(t) - F_Y^-1(t)|^p dt
//                  = sum_i sum_j w_ij |a_i - b_j|^p / (m n)   on the sorted keys a (m values) and b (n values),
//       j = floor(i n / m) .. ceil((i + 1) n / m) - 1,  w_ij = min((i + 1) n, (j + 1) m) - max(i n, j m)   (an exact integer > 0):
// the two step functions cut [0, 1] into pieces of length w_ij / (m n).  For m == n this is mean |a_(i) - b_(i)|^p, by the
// same loop.  A heading enters a block as two entries that name the same row, one cos and one sin (the chord embedding:
// continuous across +-pi); there is no wrap flag here.
//
// Numerics: float32 points in; the projection, cos / sin, the sort keys and every sum are float64 (the contract of
// sample_common.h).  Both sets are projected by the same code, so equal points give equal keys and a permuted or repeated
// set is at distance exactly 0.
//
// One launch, no float atomics.  A 256-thread group owns one (direction, block): it projects the points (thread t takes
// points t, t + 256, ..., four at a time so that an entry's row, kind, scale and direction -- all wave-uniform -- are read
// once for four coalesced row reads), sorts both key lists in dynamic LDS (bitonic, padded with +inf to the next power of
// two, both lists in the same stage loop), then thread t adds the pieces of i = t, t + 256, ... with j ascending, wave_sum,
// the four waves in order, one division.  Everything a slice reads is its own: two calls give the same bits, a block's slices
// are the same bits alone or anywhere in a table, and a direction's slice is the same bits alone or among others.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sample_common.h"

namespace {

using namespace sample_common;

constexpr int PPT = 4;                                             // points a thread projects per walk over the entries

// keys[0 .. pad) = the keys of the `cnt` columns of M along `dir`, then +inf.  Every thread walks all `d` entries in the
// first pass (base 0 < cnt), so `bad` (a row outside the matrix, a kind > 2) ends the same in every thread.
__device__ __forceinline__ void project(const float* __restrict__ M, int rows, int cnt, const int32_t* __restrict__ cols,
                                        const uint8_t* __restrict__ kind, const double* __restrict__ scale,
                                        const double* __restrict__ dir, int col_off, int d, int pad, double* __restrict__ keys,
                                        bool& bad, bool& nonfinite) {
    const int tid = threadIdx.x;
    for (int base = 0; base < pad; base += 256 * PPT) {
        double acc[PPT];
        size_t at[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int idx = base + k * 256 + tid;
            at[k] = (size_t)(idx < cnt ? idx : cnt - 1);
            acc[k] = 0.0;
        }
        const int d_pass = base < cnt ? d : 0;                     // a pass of padding only
        for (int e = 0; e < d_pass; ++e) {
            int row = cols[col_off + e];
            if (row < 0 || row >= rows) bad = true, row = 0;
            int kd = kind != nullptr ? (int)kind[col_off + e] : 0;
            if (kd > 2) bad = true, kd = 0;
            double c = dir[e];
            if (scale != nullptr) c *= scale[col_off + e];
            const float* __restrict__ r = M + (size_t)row * (size_t)cnt;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                double v = (double)r[at[k]];
                if (kd == 1) v = cos(v);
                else if (kd == 2) v = sin(v);
                acc[k] = fma(c, v, acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int idx = base + k * 256 + tid;
            if (idx < pad) {
                double key = (double)INFINITY;
                if (idx < cnt) {
                    key = acc[k];
                    if (!isfinite(key)) nonfinite = true;
                }
                keys[idx] = key;
            }
        }
    }
}

// one compare-exchange of the bitonic stage (k, j) on `keys`, pair t
__device__ __forceinline__ void exchange(double* __restrict__ keys, int t, int k, int j) {
    const int i = 2 * t - (t & (j - 1));
    const double a = keys[i], b = keys[i + j];
    const bool up = (i & k) == 0;
    if ((a > b) == up && a != b) keys[i] = b, keys[i + j] = a;
}

// grid (most directions of a block, blocks); 256 threads; dynamic LDS: pm + pn doubles
__global__ void __launch_bounds__(256) transport_kernel(const nfisam_transport_block* __restrict__ blocks, const float* __restrict__ Xt,
                                                        int x_rows, int m, int pm, const float* __restrict__ Yt, int y_rows, int n,
                                                        int pn, const int32_t* __restrict__ xcols, const int32_t* __restrict__ ycols,
                                                        const uint8_t* __restrict__ kind, const double* __restrict__ scale,
                                                        int n_entries, const double* __restrict__ dirs, long long dirs_count, int p,
                                                        double* __restrict__ out, long long out_count) {
    extern __shared__ double keys[];                               // a [pm], then b [pn]
    __shared__ double wsum[4];
    __shared__ int any_nonfinite;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y, j = blockIdx.x;
    const int col_off = blocks[b].col_off, d = blocks[b].d, nd = blocks[b].n_dirs;
    const long long dir_off = blocks[b].dir_off, out_off = blocks[b].out_off;
    if (j >= nd) return;                                           // (the whole group: blockIdx alone decides)
    if (out_off < 0 || out_off >= out_count - j) return;           // the entry has refused such a table; nothing is written
    // a block whose entries or directions leave their arrays is never walked; a row outside its matrix is replaced by row 0
    bool bad = col_off < 0 || d < 1 || (long long)col_off + d > n_entries || dir_off < 0 ||
               dir_off > dirs_count - (long long)nd * (long long)d;
    const int d_walk = bad ? 0 : d;
    const int off_walk = bad ? 0 : col_off;
    const double* __restrict__ dir = dirs + (bad ? 0 : dir_off + (long long)j * (long long)d);
    double* __restrict__ ka = keys;
    double* __restrict__ kb = keys + pm;

    if (tid == 0) any_nonfinite = 0;
    __syncthreads();
    bool nonfinite = false;
    project(Xt, x_rows, m, xcols, kind, scale, dir, off_walk, d_walk, pm, ka, bad, nonfinite);
    project(Yt, y_rows, n, ycols, kind, scale, dir, off_walk, d_walk, pn, kb, bad, nonfinite);
    if (nonfinite) any_nonfinite = 1;
    __syncthreads();
    if (bad || any_nonfinite != 0) {                               // uniform over the group: the tables and the LDS word decide
        if (tid == 0) out[out_off + j] = (double)NAN;
        return;
    }

    // bitonic sort of both lists, ascending: in the stage (k, j) compare-exchange t pairs index i (bit j clear) with i + j
    const int ha = pm >> 1, hb = pn >> 1, top = pm > pn ? pm : pn;
    for (int k = 2; k <= top; k <<= 1) {
        for (int s = k >> 1; s >= 1; s >>= 1) {
            if (k <= pm)
                for (int t = tid; t < ha; t += 256) exchange(ka, t, k, s);
            if (k <= pn)
                for (int t = tid; t < hb; t += 256) exchange(kb, t, k, s);
            __syncthreads();
        }
    }

    double sum = 0.0;
    for (int i = tid; i < m; i += 256) {
        const long long lo = (long long)i * n, hi = lo + n;
        const int j0 = (int)(lo / m), j1 = (int)((hi + m - 1) / m) - 1;
        const double ai = ka[i];
        for (int jj = j0; jj <= j1; ++jj) {
            const long long l = (long long)jj * m, h = l + m;
            const double wij = (double)((h < hi ? h : hi) - (l > lo ? l : lo));
            const double diff = fabs(ai - kb[jj]);
            sum += wij * (p == 2 ? diff * diff : diff);
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) wsum[w] = sum;
    __syncthreads();
    if (tid == 0) out[out_off + j] = waves_in_order(wsum) / ((double)m * (double)n);
}

int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

extern "C" int nfisam_sample_sliced_transport(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n,
                                              const nfisam_transport_block* blocks, const nfisam_transport_block* blocks_dev,
                                              int n_blocks, const int32_t* xcols, const int32_t* ycols, const uint8_t* kind,
                                              const double* scale, int n_entries, const double* dirs, long long dirs_count, int p,
                                              double* out, long long out_count, nfisam_stream_t stream) {
    static_assert(sizeof(nfisam_transport_block) == 32, "nfisam_transport_block is 32 bytes");
    if (Xt == nullptr || Yt == nullptr || blocks == nullptr || blocks_dev == nullptr || xcols == nullptr || ycols == nullptr ||
        dirs == nullptr || out == nullptr)
        return NFISAM_ERR_ARG;
    if (m < 1 || n < 1 || x_rows < 1 || y_rows < 1 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535) return NFISAM_ERR_ARG;
    if (m > NFISAM_TRANSPORT_MAX_N || n > NFISAM_TRANSPORT_MAX_N || (p != 1 && p != 2)) return NFISAM_ERR_ARG;
    if (dirs_count < 1 || out_count < 1) return NFISAM_ERR_ARG;
    int most = 0;
    for (int b = 0; b < n_blocks; ++b) {                           // `blocks` is the HOST copy of the table: read here only
        const long long d = blocks[b].d, nd = blocks[b].n_dirs, doff = blocks[b].dir_off, ooff = blocks[b].out_off;
        if (d < 1 || nd < 1 || nd > 65535) return NFISAM_ERR_ARG;
        if (doff < 0 || doff > dirs_count - nd * d || ooff < 0 || ooff > out_count - nd) return NFISAM_ERR_ARG;
        if (nd > most) most = (int)nd;
    }
    const int pm = next_pow2(m), pn = next_pow2(n);
    const size_t lds = (size_t)(pm + pn) * sizeof(double);
    hipError_t e = hipSuccess;
    if (lds > 48 * 1024)                                           // always the fixed maximum (see nfisam_sample_quantiles)
        e = hipFuncSetAttribute((const void*)transport_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                2 * NFISAM_TRANSPORT_MAX_N * (int)sizeof(double));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(transport_kernel, dim3((unsigned)most, (unsigned)n_blocks), dim3(256), lds, (hipStream_t)stream, blocks_dev,
                           Xt, x_rows, m, pm, Yt, y_rows, n, pn, xcols, ycols, kind, scale, n_entries, dirs, dirs_count, p, out,
                           out_count);
        e = hipGetLastError();
    }
    return launch_status(e);
}
