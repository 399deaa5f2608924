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
// does not depend on n or on its tile.
#include "factor_model.h"

namespace {

using namespace factor_model;

constexpr int MAX_SLOTS = 10;     // a mixture of four: 2 + 2 * 4
constexpr int ADD_ROWS = 8;       // second pass: loads in flight per point

// one factor at one point: g[0 .. slot_count) in the order of its rows (a's, then b's or the candidates'); `t` is wave-uniform.
// The guard comes first, as in factor_term(): a bad record yields NaN in every slot and reads nothing.
__device__ __forceinline__ void factor_score(const nfisam_factor_term* __restrict__ t, const float* __restrict__ St, size_t n,
                                             size_t pp, int total_dim, double (&g)[MAX_SLOTS]) {
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s) g[s] = NAN;
    if (!record_ok(t, total_dim)) return;
    const double* __restrict__ p = t->p;
    const float* __restrict__ A = St + (size_t)t->a * n + pp;
    const double ax = (double)A[0], ay = (double)A[n];
    switch (t->code) {
    case NFISAM_FAC_PRIOR_SE2: {
        const Se2Prior r = se2_prior_residual(ax, ay, (double)A[2 * n], p);
        double gtx, gty, gw;
        se2_tangent_score(r.tx, r.ty, r.w, p, &gtx, &gty, &gw);
        g[0] = r.c * gtx - r.s * gty, g[1] = r.s * gtx + r.c * gty, g[2] = gw;
        return;
    }
    case NFISAM_FAC_REL_SE2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        const Se2Relative r = se2_relative_residual(ax, ay, (double)A[2 * n], (double)Bv[0], (double)Bv[n], (double)Bv[2 * n], p);
        double gtx, gty, gw;
        se2_tangent_score(r.m.tx, r.m.ty, r.m.w, p, &gtx, &gty, &gw);
        const double grx = r.m.c * gtx - r.m.s * gty, gry = r.m.s * gtx + r.m.c * gty;
        const double gx = r.ci * grx - r.si * gry, gy = r.si * grx + r.ci * gry;      // d/d(x_j, y_j)
        g[0] = -gx, g[1] = -gy, g[2] = grx * r.uy - gry * r.ux - gw;        // d ux / d th_i = uy, d uy / d th_i = -ux
        g[3] = gx, g[4] = gy, g[5] = gw;
        return;
    }
    case NFISAM_FAC_RANGE: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        range_score(ax, ay, (double)Bv[0], (double)Bv[n], p[0], p[1], &g[0], &g[1]);
        g[2] = -g[0], g[3] = -g[1];
        return;
    }
    case NFISAM_FAC_RANGE_MIX: {
        const int k = t->k;
        double term[4], gx[4], gy[4];
        double top = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            term[j] = -INFINITY, gx[j] = 0.0, gy[j] = 0.0;
            if (j < k) {
                const float* __restrict__ Cv = St + (size_t)t->cand[j] * n + pp;
                const double cx = (double)Cv[0], cy = (double)Cv[n];
                term[j] = range_log_pdf(ax, ay, cx, cy, p[3 * j], p[3 * j + 1], p[3 * j + 2]);
                range_score(ax, ay, cx, cy, p[3 * j], p[3 * j + 1], &gx[j], &gy[j]);
                top = fmax(top, term[j]);
            }
        }
        double e[4], acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = (j < k) ? exp(term[j] - top) : 0.0;                                 // the largest is exp(0) = 1: acc >= 1
            acc += e[j];
        }
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < k) {
                const double r = e[j] / acc;
                sx += r * gx[j], sy += r * gy[j];
                g[2 + 2 * j] = -(r * gx[j]), g[3 + 2 * j] = -(r * gy[j]);
            }
        }
        g[0] = sx, g[1] = sy;
        return;
    }
    case NFISAM_FAC_PRIOR_R2:
        r2_score(ax - p[0], ay - p[1], p, &g[0], &g[1]);
        return;
    case NFISAM_FAC_PRIOR_R2_RANGE:
        range_score(ax, ay, p[0], p[1], p[2], p[3], &g[0], &g[1]);
        return;
    case NFISAM_FAC_REL_R2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        r2_score((double)Bv[0] - ax - p[0], (double)Bv[n] - ay - p[1], p, &g[2], &g[3]);         // d/db
        g[0] = -g[2], g[1] = -g[3];
        return;
    }
    }
}

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

// grid (tiles of 64 points, rows of G), one wave: Gt[r][p] = ((slot_0 + slot_1) + slot_2) + ... over the row's CSR list, in
// list order; ADD_ROWS loads are in flight while the adds, which cannot be reordered, run.
__global__ void __launch_bounds__(64) score_gather_kernel(const double* __restrict__ slots, int n_slots, int n,
                                                          const int32_t* __restrict__ row_off,
                                                          const int32_t* __restrict__ row_slot, double* __restrict__ Gt) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y;
    if (p >= n) return;
    const int b = row_off[r], e = row_off[r + 1];
    double s = 0.0;
    if (b < 0 || e < b || e > n_slots) {
        s = NAN;                                                       // a bad list: nothing of it is read
    } else {
        const double* __restrict__ col = slots + p;
        int i = b;
        for (; i + ADD_ROWS <= e; i += ADD_ROWS) {
            double v[ADD_ROWS];
#pragma unroll
            for (int j = 0; j < ADD_ROWS; ++j) {
                const int sl = row_slot[i + j];
                v[j] = (sl >= 0 && sl < n_slots) ? col[(size_t)sl * n] : (double)NAN;
            }
#pragma unroll
            for (int j = 0; j < ADD_ROWS; ++j) s += v[j];
        }
        for (; i < e; ++i) {
            const int sl = row_slot[i];
            s += (sl >= 0 && sl < n_slots) ? col[(size_t)sl * n] : (double)NAN;
        }
    }
    Gt[(size_t)r * n + p] = s;
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
    if (e == hipSuccess) {
        hipLaunchKernelGGL(score_gather_kernel, dim3(tiles, total_dim), dim3(64), 0, s, scratch, n_slots, n, row_off, row_slot, Gt);
        e = hipGetLastError();
    }
    return launch_status(e);
}
