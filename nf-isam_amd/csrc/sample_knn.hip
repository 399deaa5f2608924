// sample_knn.hip — a SELECTION over pairs of points: every query's k nearest neighbours within a column block, and the number
// of points inside a per-query radius.  What the Kozachenko-Leonenko entropy, the Kraskov-Stoegbauer-Grassberger mutual
// information and the Wang-Kulkarni-Verdu divergence of utils/Statistics.py are formed from on the host.
//
// Every other pair kernel of the family (sample_mmd, sample_ksd, sample_svgd, sample_modes) is a SUM over pairs; this one
// keeps, for each query, the k smallest of its n distances.  Xt [x_rows][m] holds the queries and Yt [y_rows][n] the points
// (COLUMN-major float32 device matrices, the layout of sample_common.h); entry e names row xcols[e] of Xt and row ycols[e]
// of Yt, and a block is a run of 1..16 entries (nfisam_knn_block).  For a pair (i, j) of block b
//     u_e = scale_e * wrap_e((double)x_ie - (double)y_je),      dist = max_e |u_e|   or   sqrt(sum_e u_e^2), e ascending.
//
// Numerics: float32 points in, float64 everywhere else.  The difference of two float32 values is exact in float64, so the max
// norm is one rounding (by scale) away from the real number and has no sum at all; L2 adds d products by fma, then one sqrt.
// A NaN u makes the distance NaN (the max is poisoned like the sum), and a NaN distance never enters a list; nor does an
// infinite one, which could not be told from an empty slot.
//
// knn_kernel, grid (ceil(m / 64), blocks), 256 threads: the group owns 64 queries, one per lane, the same 64 in each of the
// four waves (their coordinates sit in LDS next to the block's rows, scales and flags, so that the loop over the columns
// indexes no register array).  The n points are walked in 64-wide tiles staged as doubles in LDS; wave w takes j = 16 w ..
// 16 w + 15 of every tile (the pair-tile walk of sample_pairs.h), 16 distance accumulators a lane.  A thread keeps its KC best
// (distance, j) in registers, ascending; a candidate enters by a fully unrolled shift with compile-time indices only (KC is
// a template parameter: 4 or 16).  A wave meets its j in ascending order, so a strict `<` keeps the lower j first on equal
// distances.  The four lists of a query then meet in LDS and wave 0 merges them by (distance, j): what a query gets does not
// depend on which wave saw a point.  Nothing is summed, so nothing depends on an order -- except log_sum, the sum of
// log(k-th distance) over the queries, taken by a second launch of one group per block in the family's order: thread t adds
// queries t, t + 256, ... ascending, wave_sum, waves_in_order.  No float atomics.
// ball_kernel is the same walk with a counter in place of the lists; the four waves' counts are added in LDS (integers).
// Everything a group brings is decided by blockIdx alone: two calls give the same bits, and a block's results do not depend
// on its place in the table, on other blocks, on repeated entries, or (for one query) on m.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_pairs.h"

namespace {

using namespace sample_pairs;

constexpr int MAX_D = NFISAM_KNN_MAX_D;
constexpr int MAX_K = NFISAM_KNN_MAX_K;
static_assert(MAX_D == CH, "a block's columns are staged as one chunk");
static_assert(sizeof(nfisam_knn_block) == 16, "nfisam_knn_block is 16 bytes");

// what a block brings, the same in every thread of its groups
struct BlockHead {
    int col_off, d, radius_row;
    bool bad;                      // entries outside the lists, a row outside its matrix, d outside 1..16: never walked
};

__device__ __forceinline__ BlockHead block_head(const nfisam_knn_block* __restrict__ blocks, int b, const int32_t* __restrict__ xcols,
                                                const int32_t* __restrict__ ycols, int n_entries, int x_rows, int y_rows) {
    BlockHead h;
    h.col_off = blocks[b].col_off, h.d = blocks[b].d, h.radius_row = blocks[b].radius_row;
    h.bad = h.d < 1 || h.d > MAX_D || h.col_off < 0 || (long long)h.col_off + h.d > n_entries;
    if (!h.bad)
        for (int c = 0; c < h.d; ++c) {
            const int rx = xcols[h.col_off + c], ry = ycols[h.col_off + c];
            if (rx < 0 || rx >= x_rows || ry < 0 || ry >= y_rows) h.bad = true;
        }
    return h;
}

// the LDS a walk needs: the block's rows, scales and flags, the group's 64 queries and the staged tile of points
struct WalkShared {
    double ys[MAX_D][TILE];
    float xq[MAX_D][TILE];         // (as they are stored; converted where they are used: the difference is exact either way)
    double sc[MAX_D];
    int row_x[MAX_D], row_y[MAX_D], wrap[MAX_D];
};

// threads 0..15 bring the block's tables into LDS (a barrier of the caller publishes them)
__device__ __forceinline__ void load_tables(WalkShared& S, const BlockHead h, const int32_t* __restrict__ xcols,
                                            const int32_t* __restrict__ ycols, const double* __restrict__ scale,
                                            const uint8_t* __restrict__ wrap) {
    if (threadIdx.x < MAX_D) {
        const int c = threadIdx.x;
        const bool in = c < h.d;
        S.row_x[c] = in ? xcols[h.col_off + c] : 0;
        S.row_y[c] = in ? ycols[h.col_off + c] : 0;
        S.sc[c] = in ? (scale != nullptr ? scale[h.col_off + c] : 1.0) : 0.0;
        S.wrap[c] = in && wrap != nullptr && wrap[h.col_off + c] != 0;
    }
}

// the group's 64 queries into LDS: wave w brings columns w, w + 4, ...; a query past m is clamped (and never written out).
// The first barrier of stage_tile publishes them.
__device__ __forceinline__ void load_queries(WalkShared& S, int d, const float* __restrict__ Xt, int m, int i) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t ic = (size_t)(i < m ? i : m - 1);
    for (int c = w; c < d; c += 4) S.xq[c][lane] = Xt[(size_t)S.row_x[c] * (size_t)m + ic];
}

// tile tj of the points into LDS: wave w stages columns w, w + 4, ...; a j past n is clamped (and never used).
// Two barriers: the previous tile has been read | this one is there.
__device__ __forceinline__ void stage_tile(WalkShared& S, int d, const float* __restrict__ Yt, int n, int tj) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = tj * TILE + lane;
    const size_t jc = (size_t)(j < n ? j : n - 1);
    __syncthreads();
    for (int c = w; c < d; c += 4) S.ys[c][lane] = (double)Yt[(size_t)S.row_y[c] * (size_t)n + jc];
    __syncthreads();
}

template <int NORM, bool WRAP>
__device__ __forceinline__ void column_step(double (&acc)[JPL], double xi, const double* __restrict__ yrow, double sc) {
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) {
        double t = xi - yrow[jj];
        if (WRAP) t = wrap_pi(t);
        const double u = sc * t;
        if (NORM == NFISAM_KNN_NORM_L2) {
            acc[jj] = fma(u, u, acc[jj]);
        } else {
            const double a = fabs(u);                              // (a NaN stays: neither test replaces it afterwards)
            acc[jj] = (a > acc[jj] || a != a) ? a : acc[jj];
        }
    }
}

// acc[jj] = the distance (L2: its square) between the lane's query and point 16 w + jj of the staged tile; the columns in
// ascending order, one pass of the loop each (everything the loop reads by c lies in LDS: no register array is indexed by it)
template <int NORM>
__device__ __forceinline__ void tile_distances(double (&acc)[JPL], const WalkShared& S, int d) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int jj = 0; jj < JPL; ++jj) acc[jj] = 0.0;
#pragma unroll 1
    for (int c = 0; c < d; ++c) {
        const double xi = (double)S.xq[c][lane], sc = S.sc[c];
        const double* __restrict__ yrow = &S.ys[c][w * JPL];
        if (S.wrap[c] != 0) column_step<NORM, true>(acc, xi, yrow, sc);
        else column_step<NORM, false>(acc, xi, yrow, sc);
    }
}

// (dc, jc) into the ascending list, behind every entry of the same distance: compile-time indices only
template <int KC>
__device__ __forceinline__ void list_insert(double (&bd)[KC], int (&bj)[KC], double dc, int jc) {
    if (dc < bd[KC - 1]) {
#pragma unroll
        for (int s = KC - 1; s >= 1; --s) {
            const bool up = dc < bd[s - 1], here = dc < bd[s];     // (both read before slot s - 1 is rewritten)
            bd[s] = up ? bd[s - 1] : (here ? dc : bd[s]);
            bj[s] = up ? bj[s - 1] : (here ? jc : bj[s]);
        }
        if (dc < bd[0]) bd[0] = dc, bj[0] = jc;
    }
}

// is (bd, bj) ahead of (ad, aj) in the (distance, j) order?  An infinite distance is "none".
__device__ __forceinline__ bool ahead(double ad, int aj, double bd, int bj) {
    return bd < (double)INFINITY && (bd < ad || (bd == ad && bj < aj));
}

// grid (ceil(m / 64), n_blocks); 256 threads
template <int KC, int NORM>
__global__ void __launch_bounds__(256) knn_kernel(const nfisam_knn_block* __restrict__ blocks, const float* __restrict__ Xt, int x_rows,
                                                  int m, const float* __restrict__ Yt, int y_rows, int n, int exclude_self,
                                                  const int32_t* __restrict__ xcols, const int32_t* __restrict__ ycols,
                                                  int n_entries, const double* __restrict__ scale, const uint8_t* __restrict__ wrap,
                                                  int k, double* __restrict__ dist, int32_t* __restrict__ idx) {
    __shared__ WalkShared S;
    __shared__ double ld[4][KC][TILE];                             // the four waves' lists (KC = 16: 32 + 16 KiB)
    __shared__ int lj[4][KC][TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
    const int i = blockIdx.x * TILE + lane;
    const BlockHead h = block_head(blocks, b, xcols, ycols, n_entries, x_rows, y_rows);
    const size_t out0 = (size_t)b * (size_t)k * (size_t)m + (size_t)i;
    if (h.bad) {                                                   // (the whole group: no barrier is left waiting)
        if (w == 0 && i < m)
            for (int kk = 0; kk < k; ++kk) {
                dist[out0 + (size_t)kk * (size_t)m] = (double)NAN;
                if (idx != nullptr) idx[out0 + (size_t)kk * (size_t)m] = -1;
            }
        return;
    }
    const int d = h.d;
    load_tables(S, h, xcols, ycols, scale, wrap);
    __syncthreads();
    load_queries(S, d, Xt, m, i);

    double bd[KC];
    int bj[KC];
#pragma unroll
    for (int s = 0; s < KC; ++s) bd[s] = (double)INFINITY, bj[s] = -1;

    const int Ty = (n + TILE - 1) / TILE;
    for (int tj = 0; tj < Ty; ++tj) {
        stage_tile(S, d, Yt, n, tj);
        double acc[JPL];
        tile_distances<NORM>(acc, S, d);
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) {
            const int j = tj * TILE + w * JPL + jj;
            const double dc = NORM == NFISAM_KNN_NORM_L2 ? sqrt(acc[jj]) : acc[jj];
            if (j < n && !(exclude_self != 0 && j == i)) list_insert<KC>(bd, bj, dc, j);   // (a NaN is below nothing)
        }
    }

    // the four lists of a query meet in LDS; wave 0 merges them by (distance, j)
#pragma unroll
    for (int s = 0; s < KC; ++s) ld[w][s][lane] = bd[s], lj[w][s][lane] = bj[s];
    __syncthreads();
    if (w != 0 || i >= m) return;
    double cd[4];
    int cj[4], at[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) cd[v] = ld[v][0][lane], cj[v] = lj[v][0][lane], at[v] = 0;
    for (int kk = 0; kk < k; ++kk) {
        double wd = (double)INFINITY;
        int wj = -1, win = -1;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (ahead(wd, wj, cd[v], cj[v])) wd = cd[v], wj = cj[v], win = v;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (win == v) {                                        // the winner's list moves on (a list past its end: none)
                ++at[v];
                const bool more = at[v] < KC;
                const int s = more ? at[v] : KC - 1;
                cd[v] = more ? ld[v][s][lane] : (double)INFINITY, cj[v] = more ? lj[v][s][lane] : -1;
            }
        dist[out0 + (size_t)kk * (size_t)m] = wd;
        if (idx != nullptr) idx[out0 + (size_t)kk * (size_t)m] = wj;
    }
}

// grid (n_blocks), 256 threads: log_sum[b] = sum over the queries of log(k-th distance) where that is positive and finite,
// n_used[b] = how many; thread t adds queries t, t + 256, ... ascending, wave_sum, the four waves in order
__global__ void __launch_bounds__(256) knn_log_sum_kernel(const nfisam_knn_block* __restrict__ blocks, int x_rows, int m, int y_rows,
                                                          const int32_t* __restrict__ xcols, const int32_t* __restrict__ ycols,
                                                          int n_entries, int k, const double* __restrict__ dist,
                                                          double* __restrict__ log_sum, int32_t* __restrict__ n_used) {
    __shared__ double ps[4];
    __shared__ int pc[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x;
    const BlockHead h = block_head(blocks, b, xcols, ycols, n_entries, x_rows, y_rows);
    if (h.bad) {
        if (threadIdx.x == 0) {
            if (log_sum != nullptr) log_sum[b] = (double)NAN;
            if (n_used != nullptr) n_used[b] = 0;
        }
        return;
    }
    const double* __restrict__ eps = dist + ((size_t)b * (size_t)k + (size_t)(k - 1)) * (size_t)m;
    double s = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < m; i += 256) {
        const double e = eps[i];
        if (e > 0.0 && e < (double)INFINITY) s += log(e), ++cnt;
    }
    s = wave_sum(s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) ps[w] = s, pc[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (log_sum != nullptr) log_sum[b] = waves_in_order(ps);
        if (n_used != nullptr) n_used[b] = pc[0] + pc[1] + pc[2] + pc[3];
    }
}

// grid (ceil(m / 64), n_blocks); 256 threads
template <int NORM>
__global__ void __launch_bounds__(256) ball_kernel(const nfisam_knn_block* __restrict__ blocks, const float* __restrict__ Xt, int x_rows,
                                                   int m, const float* __restrict__ Yt, int y_rows, int n, int exclude_self,
                                                   const int32_t* __restrict__ xcols, const int32_t* __restrict__ ycols,
                                                   int n_entries, const double* __restrict__ scale, const uint8_t* __restrict__ wrap,
                                                   const double* __restrict__ radius, int n_radius, int32_t* __restrict__ count) {
    __shared__ WalkShared S;
    __shared__ int part[4][TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
    const int i = blockIdx.x * TILE + lane;
    const BlockHead h = block_head(blocks, b, xcols, ycols, n_entries, x_rows, y_rows);
    if (h.bad || h.radius_row < 0 || h.radius_row >= n_radius) {   // (the whole group: no barrier is left waiting)
        if (w == 0 && i < m) count[(size_t)b * (size_t)m + (size_t)i] = -1;
        return;
    }
    const int d = h.d;
    load_tables(S, h, xcols, ycols, scale, wrap);
    __syncthreads();
    load_queries(S, d, Xt, m, i);
    const double r = radius[(size_t)h.radius_row * (size_t)m + (size_t)(i < m ? i : m - 1)];

    int cnt = 0;
    const int Ty = (n + TILE - 1) / TILE;
    for (int tj = 0; tj < Ty; ++tj) {
        stage_tile(S, d, Yt, n, tj);
        double acc[JPL];
        tile_distances<NORM>(acc, S, d);
#pragma unroll
        for (int jj = 0; jj < JPL; ++jj) {
            const int j = tj * TILE + w * JPL + jj;
            const double dc = NORM == NFISAM_KNN_NORM_L2 ? sqrt(acc[jj]) : acc[jj];
            // strict; a NaN distance, a NaN radius and a negative radius are below nothing
            if (j < n && !(exclude_self != 0 && j == i) && dc < r) ++cnt;
        }
    }
    part[w][lane] = cnt;
    __syncthreads();
    if (w == 0 && i < m) count[(size_t)b * (size_t)m + (size_t)i] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

// the HOST copy of the table and the arguments the two entries share
bool args_ok(const void* Xt, int x_rows, int m, const void* Yt, int y_rows, int n, int exclude_self, const nfisam_knn_block* blocks,
             const void* blocks_dev, int n_blocks, const void* xcols, const void* ycols, int n_entries, int norm, int* Tx) {
    if (Xt == nullptr || Yt == nullptr || blocks == nullptr || blocks_dev == nullptr || xcols == nullptr || ycols == nullptr) return false;
    if (x_rows < 1 || y_rows < 1 || n_entries < 1 || n_blocks < 1 || n_blocks > 65535) return false;
    int Ty;
    if (!tile_count(m, Tx) || !tile_count(n, &Ty)) return false;
    if (norm != NFISAM_KNN_NORM_MAX && norm != NFISAM_KNN_NORM_L2) return false;
    if (exclude_self != 0 && m != n) return false;
    for (int b = 0; b < n_blocks; ++b)
        if (blocks[b].d < 1 || blocks[b].d > MAX_D) return false;
    return true;
}

}  // namespace

extern "C" int nfisam_sample_knn(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n, int exclude_self,
                                 const nfisam_knn_block* blocks, const nfisam_knn_block* blocks_dev, int n_blocks,
                                 const int32_t* xcols, const int32_t* ycols, int n_entries, const double* scale, const uint8_t* wrap,
                                 int k, int norm, double* dist, int32_t* idx, double* log_sum, int32_t* n_used,
                                 nfisam_stream_t stream) {
    int Tx;
    if (!args_ok(Xt, x_rows, m, Yt, y_rows, n, exclude_self, blocks, blocks_dev, n_blocks, xcols, ycols, n_entries, norm, &Tx))
        return NFISAM_ERR_ARG;
    if (dist == nullptr || k < 1 || k > MAX_K) return NFISAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)Tx, (unsigned)n_blocks), group(256);
#define NFISAM_KNN_LAUNCH(KC, NORM)                                                                                                  \
    hipLaunchKernelGGL((knn_kernel<KC, NORM>), grid, group, 0, s, blocks_dev, Xt, x_rows, m, Yt, y_rows, n, exclude_self, xcols, ycols, \
                       n_entries, scale, wrap, k, dist, idx)
    if (norm == NFISAM_KNN_NORM_MAX) {
        if (k <= 4) NFISAM_KNN_LAUNCH(4, NFISAM_KNN_NORM_MAX);
        else NFISAM_KNN_LAUNCH(MAX_K, NFISAM_KNN_NORM_MAX);
    } else {
        if (k <= 4) NFISAM_KNN_LAUNCH(4, NFISAM_KNN_NORM_L2);
        else NFISAM_KNN_LAUNCH(MAX_K, NFISAM_KNN_NORM_L2);
    }
#undef NFISAM_KNN_LAUNCH
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && (log_sum != nullptr || n_used != nullptr)) {
        hipLaunchKernelGGL(knn_log_sum_kernel, dim3((unsigned)n_blocks), group, 0, s, blocks_dev, x_rows, m, y_rows, xcols, ycols,
                           n_entries, k, dist, log_sum, n_used);
        e = hipGetLastError();
    }
    return launch_status(e);
}

extern "C" int nfisam_sample_ball_count(const float* Xt, int x_rows, int m, const float* Yt, int y_rows, int n, int exclude_self,
                                        const nfisam_knn_block* blocks, const nfisam_knn_block* blocks_dev, int n_blocks,
                                        const int32_t* xcols, const int32_t* ycols, int n_entries, const double* scale,
                                        const uint8_t* wrap, int norm, const double* radius, int n_radius, int32_t* count,
                                        nfisam_stream_t stream) {
    int Tx;
    if (!args_ok(Xt, x_rows, m, Yt, y_rows, n, exclude_self, blocks, blocks_dev, n_blocks, xcols, ycols, n_entries, norm, &Tx))
        return NFISAM_ERR_ARG;
    if (radius == nullptr || count == nullptr || n_radius < 1) return NFISAM_ERR_ARG;
    for (int b = 0; b < n_blocks; ++b)
        if (blocks[b].radius_row < 0 || blocks[b].radius_row >= n_radius) return NFISAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)Tx, (unsigned)n_blocks), group(256);
    if (norm == NFISAM_KNN_NORM_MAX)
        hipLaunchKernelGGL((ball_kernel<NFISAM_KNN_NORM_MAX>), grid, group, 0, s, blocks_dev, Xt, x_rows, m, Yt, y_rows, n, exclude_self,
                           xcols, ycols, n_entries, scale, wrap, radius, n_radius, count);
    else
        hipLaunchKernelGGL((ball_kernel<NFISAM_KNN_NORM_L2>), grid, group, 0, s, blocks_dev, Xt, x_rows, m, Yt, y_rows, n, exclude_self,
                           xcols, ycols, n_entries, scale, wrap, radius, n_radius, count);
    return launch_status(hipGetLastError());
}
