// factor_hessian.hip — Hessian-vector products of the factor graph's joint density:
//     Ht[r][p] = sum_c  d^2 log p / dx_r dx_c (X_p) * Vt[c][p]
// the third row of value / score / curvature, written from the same residuals and terms (factor_model.h).  A dense Hessian is
// total_dim^2 per point and would be assembled with atomics; a factor's contribution to H v is ONE number per row the factor
// reads -- the slot layout of factor_score.hip, so its gather lists (slot_off, row_off / row_slot) serve unchanged.
//
// What is differentiated: the SMOOTH float64 formula whose gradient factor_score() evaluates, at the float32 point, along the
// float64 direction v: every line of the score once more with its derivative along v next to it (se2_tangent_hvp, range_hvp;
// the rotations and d u / d th_i = (uy, -ux) of the residuals here).  At a range of exactly 0, where the score is the zero
// vector, the product is the zero vector too.  A mixture with softmax weights r_j (shifted by the largest term, as in value
// and score), component gradients g_j and Hessians H_j:  H v = sum_j r_j (H_j v + g_j (g_j . v)) - g (g . v),  g = sum_j r_j g_j;
// with s_j = g_j . v and S = sum_j r_j s_j = g . v this is, on candidate j's rows, -m_j with m_j = r_j (H_j q_j + g_j (s_j - S))
// (g_j and H_j in the pose's rows, q_j = v_pose - v_cand_j) and sum_j m_j on the pose's rows: finite wherever the terms are.
//
// Launch form and contract: those of factor_score.hip.  (1) a wave per (64-point tile, run of FAC_RUN factors), code and
// parameters wave-uniform, writes slot_count() slots per factor into scratch [n_slots][n]; with a score asked for, the same
// pass also writes factor_score()'s slots into a second scratch [n_slots][n] behind the first -- the SAME device function
// on the same inputs, so Gt has nfisam_factor_graph_score's bits.  (2) the shared gather (factor_slots.h) adds a row's slots in
// table order, once per result.  No float atomics; two calls give the same bits; a point's column does not depend on n or on
// its tile; record_ok() is the one guard: a bad record reads nothing (neither St nor Vt) and owns NaN in its slots.
#include "factor_slots.h"

namespace {

using namespace factor_model;

// one factor at one point: hv[0 .. slot_count) = (H_f v) in the order of the factor's rows; `t` is wave-uniform
__device__ __forceinline__ void factor_hvp(const nfisam_factor_term* __restrict__ t, const float* __restrict__ St,
                                           const double* __restrict__ Vt, size_t n, size_t pp, int total_dim,
                                           double (&hv)[MAX_SLOTS]) {
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s) hv[s] = NAN;
    if (!record_ok(t, total_dim)) return;
    const double* __restrict__ p = t->p;
    const float* __restrict__ A = St + (size_t)t->a * n + pp;
    const double* __restrict__ VA = Vt + (size_t)t->a * n + pp;
    const double ax = (double)A[0], ay = (double)A[n];
    const double vax = VA[0], vay = VA[n];
    switch (t->code) {
    case NFISAM_FAC_PRIOR_SE2: {
        const Se2Prior r = se2_prior_residual(ax, ay, (double)A[2 * n], p);
        double gtx, gty, htx, hty, hw;
        se2_tangent_hvp(r.tx, r.ty, r.w, p, r.c * vax + r.s * vay, r.c * vay - r.s * vax, VA[2 * n], &gtx, &gty, &htx, &hty, &hw);
        hv[0] = r.c * htx - r.s * hty, hv[1] = r.s * htx + r.c * hty, hv[2] = hw;
        return;
    }
    case NFISAM_FAC_REL_SE2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        const double* __restrict__ VB = Vt + (size_t)t->b * n + pp;
        const Se2Relative r = se2_relative_residual(ax, ay, (double)A[2 * n], (double)Bv[0], (double)Bv[n], (double)Bv[2 * n], p);
        const double vthi = VA[2 * n], ddx = VB[0] - vax, ddy = VB[n] - vay;
        const double dux = r.ci * ddx + r.si * ddy + r.uy * vthi, duy = r.ci * ddy - r.si * ddx - r.ux * vthi;    // d u along v
        double gtx, gty, htx, hty, hw;
        se2_tangent_hvp(r.m.tx, r.m.ty, r.m.w, p, r.m.c * dux + r.m.s * duy, r.m.c * duy - r.m.s * dux, VB[2 * n] - vthi, &gtx, &gty,
                        &htx, &hty, &hw);
        const double grx = r.m.c * gtx - r.m.s * gty, gry = r.m.s * gtx + r.m.c * gty;          // d/du and its derivative along v
        const double hrx = r.m.c * htx - r.m.s * hty, hry = r.m.s * htx + r.m.c * hty;
        // d/d(x_j, y_j) = R(th_i) d/du: the rotation turns with th_i
        const double hx = r.ci * hrx - r.si * hry - (r.si * grx + r.ci * gry) * vthi;
        const double hy = r.si * hrx + r.ci * hry + (r.ci * grx - r.si * gry) * vthi;
        hv[0] = -hx, hv[1] = -hy, hv[2] = hrx * r.uy + grx * duy - hry * r.ux - gry * dux - hw;
        hv[3] = hx, hv[4] = hy, hv[5] = hw;
        return;
    }
    case NFISAM_FAC_RANGE: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        const double* __restrict__ VB = Vt + (size_t)t->b * n + pp;
        range_hvp(ax, ay, (double)Bv[0], (double)Bv[n], p[0], p[1], vax - VB[0], vay - VB[n], &hv[0], &hv[1]);
        hv[2] = -hv[0], hv[3] = -hv[1];
        return;
    }
    case NFISAM_FAC_RANGE_MIX: {
        const int k = t->k;
        double term[4], gx[4], gy[4], hx[4], hy[4], sj[4];
        double top = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            term[j] = -INFINITY, gx[j] = 0.0, gy[j] = 0.0, hx[j] = 0.0, hy[j] = 0.0, sj[j] = 0.0;
            if (j < k) {
                const float* __restrict__ Cv = St + (size_t)t->cand[j] * n + pp;
                const double* __restrict__ VC = Vt + (size_t)t->cand[j] * n + pp;
                const double cx = (double)Cv[0], cy = (double)Cv[n];
                const double qx = vax - VC[0], qy = vay - VC[n];
                term[j] = range_log_pdf(ax, ay, cx, cy, p[3 * j], p[3 * j + 1], p[3 * j + 2]);
                range_score(ax, ay, cx, cy, p[3 * j], p[3 * j + 1], &gx[j], &gy[j]);
                range_hvp(ax, ay, cx, cy, p[3 * j], p[3 * j + 1], qx, qy, &hx[j], &hy[j]);
                sj[j] = gx[j] * qx + gy[j] * qy;                                       // g_j . v
                top = fmax(top, term[j]);
            }
        }
        double e[4], acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            e[j] = (j < k) ? exp(term[j] - top) : 0.0;                                 // the largest is exp(0) = 1: acc >= 1
            acc += e[j];
        }
        double S = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < k) S += e[j] / acc * sj[j];                                        // g . v
        double mx = 0.0, my = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < k) {
                const double r = e[j] / acc;
                const double cx = r * (hx[j] + gx[j] * (sj[j] - S)), cy = r * (hy[j] + gy[j] * (sj[j] - S));
                mx += cx, my += cy;
                hv[2 + 2 * j] = -cx, hv[3 + 2 * j] = -cy;
            }
        }
        hv[0] = mx, hv[1] = my;
        return;
    }
    case NFISAM_FAC_PRIOR_R2:
        r2_score(vax, vay, p, &hv[0], &hv[1]);                                         // -P v: the constant block
        return;
    case NFISAM_FAC_PRIOR_R2_RANGE:
        range_hvp(ax, ay, p[0], p[1], p[2], p[3], vax, vay, &hv[0], &hv[1]);
        return;
    case NFISAM_FAC_REL_R2: {
        const double* __restrict__ VB = Vt + (size_t)t->b * n + pp;
        r2_score(VB[0] - vax, VB[n] - vay, p, &hv[2], &hv[3]);                         // -P (v_b - v_a): the rows of b
        hv[0] = -hv[2], hv[1] = -hv[3];
        return;
    }
    }
}

// grid (tiles of 64 points, runs of FAC_RUN factors), one wave per block; SCORE: factor_score()'s slots go behind H v's
template <bool SCORE>
__global__ void __launch_bounds__(64) factor_hvp_kernel(const nfisam_factor_term* __restrict__ terms, int n_terms,
                                                        const float* __restrict__ St, const double* __restrict__ Vt,
                                                        int total_dim, int n, const int32_t* __restrict__ slot_off, int n_slots,
                                                        double* __restrict__ slots) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    const size_t pp = (p < n) ? (size_t)p : (size_t)(n - 1);
    const int f1 = min((int)(blockIdx.y + 1) * FAC_RUN, n_terms);
    for (int f = blockIdx.y * FAC_RUN; f < f1; ++f) {
        double hv[MAX_SLOTS], g[MAX_SLOTS];
        factor_hvp(terms + f, St, Vt, (size_t)n, pp, total_dim, hv);
        if (SCORE) factor_score(terms + f, St, (size_t)n, pp, total_dim, g);
        const int cnt = slot_count(terms[f].code, terms[f].k);
        const int s0 = slot_off[f];
        if (s0 < 0 || (long long)s0 + cnt > n_slots) continue;         // slots outside the scratch: nothing is written
        if (p < n) {
#pragma unroll
            for (int s = 0; s < MAX_SLOTS; ++s)
                if (s < cnt) {
                    slots[(size_t)(s0 + s) * n + p] = hv[s];
                    if (SCORE) slots[((size_t)n_slots + s0 + s) * n + p] = g[s];
                }
        }
    }
}

}  // namespace

extern "C" size_t nfisam_factor_graph_hvp_scratch_count(int n_slots, int n, int with_score) {
    if (n_slots < 0 || n < 0) return 0;
    return (size_t)n_slots * (size_t)n * (with_score ? 2 : 1);        // one double per (slot, point) and result
}

extern "C" int nfisam_factor_graph_hvp(const nfisam_factor_term* terms, int n_terms, const float* St, const double* Vt,
                                       int total_dim, int n, const int32_t* slot_off, int n_slots, const int32_t* row_off,
                                       const int32_t* row_slot, double* Ht, double* Gt, double* scratch, nfisam_stream_t stream) {
    if (St == nullptr || Vt == nullptr || Ht == nullptr || n_terms < 0 || n < 0 || total_dim < 1 || n_slots < 0) return NFISAM_ERR_ARG;
    if (n_terms > 0 && (terms == nullptr || slot_off == nullptr || row_off == nullptr || row_slot == nullptr || scratch == nullptr))
        return NFISAM_ERR_ARG;
    if (fac_runs(n_terms) > GRID_Y_MAX || total_dim > GRID_Y_MAX) return NFISAM_ERR_ARG;
    if ((long long)n_slots > (long long)MAX_SLOTS * n_terms) return NFISAM_ERR_ARG;
    if (n == 0) return NFISAM_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)total_dim * n * sizeof(double);
    if (n_terms == 0) {                                                // the empty graph: a zero product, a zero score
        hipError_t e = hipMemsetAsync(Ht, 0, bytes, s);
        if (e == hipSuccess && Gt != nullptr) e = hipMemsetAsync(Gt, 0, bytes, s);
        return launch_status(e);
    }
    const dim3 grid((n + 63) / 64, fac_runs(n_terms));
    if (Gt != nullptr)
        hipLaunchKernelGGL(factor_hvp_kernel<true>, grid, dim3(64), 0, s, terms, n_terms, St, Vt, total_dim, n, slot_off, n_slots, scratch);
    else
        hipLaunchKernelGGL(factor_hvp_kernel<false>, grid, dim3(64), 0, s, terms, n_terms, St, Vt, total_dim, n, slot_off, n_slots, scratch);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_gather(scratch, n_slots, n, total_dim, row_off, row_slot, Ht, s);
    if (e == hipSuccess && Gt != nullptr)
        e = launch_gather(scratch + (size_t)n_slots * n, n_slots, n, total_dim, row_off, row_slot, Gt, s);
    return launch_status(e);
}
