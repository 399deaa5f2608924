// factor_density.hip — the joint log-density of the factor graph, log p(X, Z) = sum_f log p_f(x_f), at n points.
//
// The reference evaluates it with per-sample Python loops over SE2Pose objects (src/factors/Factors.py `log_pdf` of every
// class, summed by JointFactor.log_pdf, src/sampler/sampler_utils.py:85-98).  Here a factor is one fixed-size record of a
// device table (nfisam_factor_term) and the points are the column-major float32 sample matrix St[total_dim][n] that the
// tree walk writes: a posterior draw is scored where it lies.
//
// Numerics: the contract of sample_common.h.  The bundled graphs pin the first pose with heading variances down to 1e-12 and
// their joint values reach 1e4..1e11: every residual, quadratic form, log-sum-exp and both sums are double, like the parameters.
//
// Two launches.  (1) a wave owns a 64-point tile and a contiguous run of FAC_RUN factors: the factor index depends on the
// block index alone, so the code and every parameter are wave-uniform (scalar loads, no divergence inside the wave), each
// variable row is one coalesced 256-byte read, and the tile's rows are re-read from cache along the run; terms go to
// per_factor[f][p].  (2) per 64-point tile the terms are added strictly in table order (see factor_sum_kernel):
// log_p[p] is the left-to-right float64 sum of per_factor[0..n_terms)[p], whatever n and whichever tile p falls in.  No
// float atomics: two calls give the same bits.
#include "factor_model.h"

namespace {

using namespace factor_model;

constexpr int SUM_WAVES = 16;     // second pass: waves per 64-point tile ...
constexpr int SUM_ROWS = 8;       // ... and rows each of them has in flight per stage (16 x 8 x 64 doubles = 64 KB of LDS)

// one factor at one point; `t` is wave-uniform.  pp = the point's column of St (clamped: lanes past n compute and drop).
// The guard comes first (wave-uniform, scalar): a bad table yields NaN, never a stray read.
__device__ __forceinline__ double factor_term(const nfisam_factor_term* __restrict__ t, const float* __restrict__ St, size_t n,
                                              size_t pp, int total_dim) {
    if (!record_ok(t, total_dim)) return NAN;
    const double* __restrict__ p = t->p;
    const float* __restrict__ A = St + (size_t)t->a * n + pp;
    const double ax = (double)A[0], ay = (double)A[n];
    switch (t->code) {
    case NFISAM_FAC_PRIOR_SE2: {
        const Se2Prior r = se2_prior_residual(ax, ay, (double)A[2 * n], p);
        return se2_tangent_log_pdf(r.tx, r.ty, r.w, p);
    }
    case NFISAM_FAC_REL_SE2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        const Se2Relative r = se2_relative_residual(ax, ay, (double)A[2 * n], (double)Bv[0], (double)Bv[n], (double)Bv[2 * n], p);
        return se2_tangent_log_pdf(r.m.tx, r.m.ty, r.m.w, p);
    }
    case NFISAM_FAC_RANGE: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        return range_log_pdf(ax, ay, (double)Bv[0], (double)Bv[n], p[0], p[1], p[2]);
    }
    case NFISAM_FAC_RANGE_MIX: {
        const int k = t->k;
        double term[4], top = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < k) {
                const float* __restrict__ Cv = St + (size_t)t->cand[j] * n + pp;
                term[j] = range_log_pdf(ax, ay, (double)Cv[0], (double)Cv[n], p[3 * j], p[3 * j + 1], p[3 * j + 2]);
                top = fmax(top, term[j]);
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < k) acc += exp(term[j] - top);
        return top + log(acc);
    }
    case NFISAM_FAC_PRIOR_R2:
        return r2_log_pdf(ax - p[0], ay - p[1], p);
    case NFISAM_FAC_PRIOR_R2_RANGE:
        return range_log_pdf(ax, ay, p[0], p[1], p[2], p[3], p[4]);
    case NFISAM_FAC_REL_R2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        return r2_log_pdf((double)Bv[0] - ax - p[0], (double)Bv[n] - ay - p[1], p);
    }
    }
    return NAN;
}

// grid (tiles of 64 points, runs of FAC_RUN factors), one wave per block
__global__ void __launch_bounds__(64) factor_terms_kernel(const nfisam_factor_term* __restrict__ terms, int n_terms,
                                                          const float* __restrict__ St, int total_dim, int n,
                                                          double* __restrict__ per) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    const size_t pp = (p < n) ? (size_t)p : (size_t)(n - 1);
    const int f1 = min((int)(blockIdx.y + 1) * FAC_RUN, n_terms);
    for (int f = blockIdx.y * FAC_RUN; f < f1; ++f) {
        const double v = factor_term(terms + f, St, (size_t)n, pp, total_dim);
        if (p < n) per[(size_t)f * n + p] = v;
    }
}

// log_p[p] = ((per[0][p] + per[1][p]) + per[2][p]) + ... : strictly table order, one accumulator per point.  The chain of
// n_terms dependent adds cannot be split without changing the rounding, so the block hides the LOADS instead: 16 waves own a
// 64-point tile; per stage wave w fetches SUM_ROWS rows (16 x 8 = 128 rows in flight per point), parks them in LDS, and wave 0
// adds the stage's rows in order while everybody's loads of the next stage are already under way (the registers are the
// second buffer).  (One wave with 32 loads in flight took 34 us for 1584 factors at n = 500 -- 2/3 of the call.)
__global__ void __launch_bounds__(64 * SUM_WAVES) factor_sum_kernel(const double* __restrict__ per, int n_terms, int n,
                                                                   double* __restrict__ log_p) {
    __shared__ double buf[SUM_WAVES * SUM_ROWS][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    const double* __restrict__ col = per + ((p < n) ? p : n - 1);
    constexpr int STAGE = SUM_WAVES * SUM_ROWS;
    double v[SUM_ROWS];
#pragma unroll
    for (int j = 0; j < SUM_ROWS; ++j) {
        const int f = w * SUM_ROWS + j;
        v[j] = (f < n_terms) ? col[(size_t)f * n] : 0.0;
    }
    double s = 0.0;
    for (int f0 = 0; f0 < n_terms; f0 += STAGE) {
#pragma unroll
        for (int j = 0; j < SUM_ROWS; ++j) buf[w * SUM_ROWS + j][lane] = v[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SUM_ROWS; ++j) {                 // the next stage's loads, in flight during the adds below
            const int f = f0 + STAGE + w * SUM_ROWS + j;
            v[j] = (f < n_terms) ? col[(size_t)f * n] : 0.0;
        }
        if (w == 0) {
            const int cnt = min(STAGE, n_terms - f0);
            int r = 0;
            for (; r + 8 <= cnt; r += 8) {
                double t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = buf[r + j][lane];
#pragma unroll
                for (int j = 0; j < 8; ++j) s += t[j];
            }
            for (; r < cnt; ++r) s += buf[r][lane];
        }
        __syncthreads();
    }
    if (w == 0 && p < n) log_p[p] = s;
}

}  // namespace

extern "C" int nfisam_factor_graph_log_density(const nfisam_factor_term* terms, int n_terms, const float* St, int total_dim,
                                               int n, double* log_p, double* per_factor, nfisam_stream_t stream) {
    if (terms == nullptr || St == nullptr || log_p == nullptr || n_terms < 0 || n < 0 || total_dim < 1) return NFISAM_ERR_ARG;
    if (fac_runs(n_terms) > GRID_Y_MAX) return NFISAM_ERR_ARG;
    if (n == 0) return NFISAM_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (n_terms == 0)                                          // the empty graph: log p = 0
        return launch_status(hipMemsetAsync(log_p, 0, (size_t)n * sizeof(double), s));
    double* per = per_factor;
    if (per == nullptr) {
        e = hipMallocAsync((void**)&per, (size_t)n_terms * n * sizeof(double), s);
        if (e != hipSuccess) return launch_status(e);
    }
    const int tiles = (n + 63) / 64;
    hipLaunchKernelGGL(factor_terms_kernel, dim3(tiles, fac_runs(n_terms)), dim3(64), 0, s, terms, n_terms, St, total_dim, n, per);
    e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(factor_sum_kernel, dim3(tiles), dim3(64 * SUM_WAVES), 0, s, per, n_terms, n, log_p);
        e = hipGetLastError();
    }
    int rc = launch_status(e);
    if (per_factor == nullptr) {
        e = hipFreeAsync(per, s);
        if (rc == NFISAM_OK) rc = launch_status(e);
    }
    return rc;
}
