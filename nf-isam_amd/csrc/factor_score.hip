// factor_score.hip — the score of the factor graph's joint density, G[r][p] = d/dx_r log p(X, Z) at point p.
//
// The reference has `grad_x_log_pdf` on every factor class (src/factors/Factors.py:829-850, :1450-1478, :2203-2223,
// :2732-2751, :3135-3156) and adds them per variable in JointFactor.grad_x_log_pdf (src/sampler/sampler_utils.py:100-113),
// sample by sample in Python; its one consumer is the kernel Stein discrepancy (src/utils/Statistics.py:193-245).  Here the
// factors are the table of factor_density.hip (nfisam_factor_term, the same seven codes) and the points are the column-major
// float32 matrix St[total_dim][n]; the result is the float64 column-major matrix Gt[total_dim][n].
//
// Numerics: the contract of sample_common.h.  Value and score are written from the same residuals and terms (factor_model.h):
// this is the derivative of the float64 formula that factor_term() of factor_density.hip evaluates, at the float32 point -- of
// the SMOOTH formula everywhere: the value's own branches (|w| < 1e-10 in the log map, |w| < 1e-5 in its Jacobian) are flat
// spots of 1e-10 and get no derivative-zero plateaus.  A mixture's derivative is sum_j r_j grad term_j with r the softmax of
// the component terms, shifted by their maximum like the value's log-sum-exp: finite wherever the terms are.
//
// Two launches, no float atomics.  (1) like factor_terms_kernel: a wave owns a 64-point tile and a run of FAC_RUN factors,
// code and parameters wave-uniform; factor f writes its slot_count() partial derivatives into its own slots slot_off[f] .. of
// the scratch [n_slots][n], in the order of the factor's rows: a, then b or the candidates.  (2) a wave per (64-point tile,
// row r of G) adds the slots row_slot[row_off[r] .. row_off[r + 1]) in that order -- the host lists a row's slots in table
// order -- one accumulator per point.  A row without a slot is 0.  Hence: two calls give the same bits, and a point's column
// does not depend on n or on its tile.  factor_score() and the gather live in factor_slots.h: factor_hessian.hip shares both.
#include "factor_slots.h"

namespace {

using namespace factor_model;

// grid (tiles of 64 points, runs of FAC_RUN factors), one wave per block
__global__ void __launch_bounds__(64) factor_score_kernel(const nfisam_factor_term* __restrict__ terms, int n_terms,
                                                          const float* __restrict__ St, int total_dim, int n,
                                                          const int32_t* __restrict__ slot_off, int n_slots,
                                                          double* __restrict__ slots) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    const size_t pp = (p < n) ? (size_t)p : (size_t)(n - 1);
    const int f1 = min((int)(blockIdx.y + 1) * FAC_RUN, n_terms);
    for (int f = blockIdx.y * FAC_RUN; f < f1; ++f) {
        double g[MAX_SLOTS];
        factor_score(terms + f, St, (size_t)n, pp, total_dim, g);
        const int cnt = slot_count(terms[f].code, terms[f].k);
        const int s0 = slot_off[f];
        if (s0 < 0 || (long long)s0 + cnt > n_slots) continue;         // slots outside the scratch: nothing is written
        if (p < n) {
#pragma unroll
            for (int s = 0; s < MAX_SLOTS; ++s)
                if (s < cnt) slots[(size_t)(s0 + s) * n + p] = g[s];
        }
    }
}

}  // namespace

extern "C" size_t nfisam_factor_graph_score_scratch_count(int n_slots, int n) {
    if (n_slots < 0 || n < 0) return 0;
    return (size_t)n_slots * (size_t)n;                                // one double per (slot, point)
}

extern "C" int nfisam_factor_graph_score(const nfisam_factor_term* terms, int n_terms, const float* St, int total_dim, int n,
                                         const int32_t* slot_off, int n_slots, const int32_t* row_off, const int32_t* row_slot,
                                         double* Gt, double* scratch, nfisam_stream_t stream) {
    if (St == nullptr || Gt == nullptr || n_terms < 0 || n < 0 || total_dim < 1 || n_slots < 0) return NFISAM_ERR_ARG;
    if (n_terms > 0 && (terms == nullptr || slot_off == nullptr || row_off == nullptr || row_slot == nullptr || scratch == nullptr))
        return NFISAM_ERR_ARG;
    if (fac_runs(n_terms) > GRID_Y_MAX || total_dim > GRID_Y_MAX) return NFISAM_ERR_ARG;
    if ((long long)n_slots > (long long)MAX_SLOTS * n_terms) return NFISAM_ERR_ARG;
    if (n == 0) return NFISAM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n_terms == 0)                                                  // the empty graph: a zero score
        return launch_status(hipMemsetAsync(Gt, 0, (size_t)total_dim * n * sizeof(double), s));
    const int tiles = (n + 63) / 64;
    hipLaunchKernelGGL(factor_score_kernel, dim3(tiles, fac_runs(n_terms)), dim3(64), 0, s, terms, n_terms, St, total_dim, n,
                       slot_off, n_slots, scratch);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_gather(scratch, n_slots, n, total_dim, row_off, row_slot, Gt, s);
    return launch_status(e);
}
