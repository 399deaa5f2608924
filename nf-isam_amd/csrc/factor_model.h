// factor_model.h — the factor model that factor_density.hip (the value), factor_score.hip (its gradient) and factor_hessian.hip
// (its Hessian-vector product) share, once each:
// what a record of the table (nfisam_factor_term, the seven NFISAM_FAC_* codes) reads, the ONE guard in front of every read,
// the residuals and the per-term formulas.  A new evaluator of the factors starts here.  Numerics and layout: the contract of
// sample_common.h.  `t` and `p` are wave-uniform (the factor index depends on the block index alone) and `const __restrict__`:
// the code, the rows and every parameter are scalar loads, the guard is a scalar branch.
#pragma once
#include "sample_common.h"

namespace factor_model {

using namespace sample_common;

constexpr int FAC_RUN = 8;        // factors per wave in an evaluator's first pass: grid (64-point tiles, runs of FAC_RUN)
constexpr int GRID_Y_MAX = 65535; // the grid's second dimension
inline int fac_runs(int n_terms) { return (n_terms + FAC_RUN - 1) / FAC_RUN; }

// rows of St a record reads at `a` and at `b` (0: `b` is not read), for a code in range
__device__ __forceinline__ int rows_a(int code) { return (code == NFISAM_FAC_PRIOR_SE2 || code == NFISAM_FAC_REL_SE2) ? 3 : 2; }
__device__ __forceinline__ int rows_b(int code) {
    return code == NFISAM_FAC_REL_SE2 ? 3 : (code == NFISAM_FAC_RANGE || code == NFISAM_FAC_REL_R2) ? 2 : 0;
}

// the slots (partial derivatives) a record owns: one per row it reads; none where a code or a k out of range leaves that open
__device__ __forceinline__ int slot_count(int code, int k) {
    if (code < NFISAM_FAC_PRIOR_SE2 || code > NFISAM_FAC_REL_R2) return 0;
    if (code == NFISAM_FAC_RANGE_MIX) return (k >= 1 && k <= 4) ? 2 + 2 * k : 0;
    return rows_a(code) + rows_b(code);
}

// THE guard: the code, the rows at `a` and `b`, a mixture's k and every used candidate against total_dim (>= 1).  Called
// before any address is formed: a bad record reads nothing and yields NaN (its term, the slots it owns).
__device__ __forceinline__ bool record_ok(const nfisam_factor_term* __restrict__ t, int total_dim) {
    const int code = t->code, a = t->a, b = t->b, k = t->k;           // the record's head, read whole: one scalar load
    if (code < NFISAM_FAC_PRIOR_SE2 || code > NFISAM_FAC_REL_R2) return false;
    if (a < 0 || a > total_dim - rows_a(code)) return false;
    if (rows_b(code) > 0 && (b < 0 || b > total_dim - rows_b(code))) return false;
    if (code == NFISAM_FAC_RANGE_MIX) {
        if (k < 1 || k > 4) return false;
        const int c[4] = {t->cand[0], t->cand[1], t->cand[2], t->cand[3]};
        for (int j = 0; j < 4; ++j)
            if (j < k && (c[j] < 0 || c[j] > total_dim - 2)) return false;
    }
    return true;
}

// ---- SE(2).  The residual dT = (tx, ty, w) = p[0:3]^-1 * (x, y, th), with the rotation (s, c) into the measurement's frame:
// the value ignores it, the score rotates its gradient back with it.
struct Se2Prior { double tx, ty, w, s, c; };
__device__ __forceinline__ Se2Prior se2_prior_residual(double x, double y, double th, const double* __restrict__ p) {
    Se2Prior r;
    sincos(p[2], &r.s, &r.c);
    const double dx = x - p[0], dy = y - p[1];
    r.w = wrap_pi(wrap_pi(-p[2]) + wrap_pi(th));
    r.tx = r.c * dx + r.s * dy, r.ty = r.c * dy - r.s * dx;
    return r;
}

// p[0:3]^-1 * (a^-1 * b): the prior's residual `m` of b in pose a's frame, (ux, uy) = R(th_a)' (b - a) with (si, ci) of th_a
struct Se2Relative { Se2Prior m; double si, ci, ux, uy; };
__device__ __forceinline__ Se2Relative se2_relative_residual(double ax, double ay, double thi, double bx, double by, double thj,
                                                             const double* __restrict__ p) {
    Se2Relative r;
    sincos(thi, &r.si, &r.ci);
    const double dx = bx - ax, dy = by - ay;
    r.ux = r.ci * dx + r.si * dy, r.uy = r.ci * dy - r.si * dx;
    r.m = se2_prior_residual(r.ux, r.uy, wrap_pi(-wrap_pi(thi)) + wrap_pi(thj), p);
    return r;
}

// log N(Log(dT); 0, Sigma) + log|det dLog| for dT = (tx, ty, w); p[3..8] = upper triangle of the precision, p[9] = log normaliser.
// Log: v = V^-1(w) t with V^-1 = [[a, w/2], [-w/2, a]], a = (w/2) cot(w/2) (the half-angle form of
// geometry/TwoDimension.py:405-418); det dLog = w^2 / (4 sin^2(w/2)), 1 for |w| < 1e-5 (:437-441).  Below |w| = 1e-10 only a
// is set to 1 (it is 1 - w^2 / 12 there); the off-diagonal w/2 stays: the reference's identity drops a term of |w| |t| / 2,
// 1e-10 relative and 7e4 roundings against tests/golden/factor_exact.npz (profiles/factor_exact.json).
__device__ __forceinline__ double se2_tangent_log_pdf(double tx, double ty, double w, const double* __restrict__ p) {
    const double h = 0.5 * w;
    double sh, ch;
    sincos(h, &sh, &ch);
    const bool small = fabs(w) < 1e-10;
    const double a = small ? 1.0 : h * ch / sh;
    const double vx = a * tx + h * ty, vy = a * ty - h * tx;
    const double q = p[3] * vx * vx + p[6] * vy * vy + p[8] * w * w + 2.0 * (p[4] * vx * vy + p[5] * vx * w + p[7] * vy * w);
    const double log_det = (fabs(w) < 1e-5) ? 0.0 : 2.0 * log(fabs(h / sh));
    return p[9] - 0.5 * q + log_det;
}

// a(h) = h cot h, its derivative in w = 2h, a'(w) = (cot h - h / sin^2 h) / 2, and the derivative of the log-det term
// 2 log|h / sin h| in w, l'(w) = 1 / h - cot h.  Both derivatives are differences of two terms of size 1 / h that leave
// 2h / 3 resp. h / 3: the plain forms lose 1.5 eps / h^2 relative (six digits left at h = 1e-5).  Below SERIES_H the Taylor
// series in h, through h^9, are used instead (coefficients: 2^2k |B_2k| / (2k)!).  The threshold balances the two errors:
// at h = 0.1 the plain forms have lost 1.5 eps / h^2 = 1.7e-14 (two digits) and the first dropped terms, 1.3e-5 h^11 and
// 2.2e-6 h^11 against h / 3, are 3.9e-15 and 6.5e-16 relative -- neither side of the switch is more than about two digits
// worse than the other, and further from the switch each side only improves.
constexpr double SERIES_H = 0.1;

__device__ __forceinline__ void log_map_terms(double w, double* a, double* da_dw, double* dlogdet_dw) {
    const double h = 0.5 * w;
    if (fabs(h) < SERIES_H) {
        const double h2 = h * h;
        *a = 1.0 - h2 * (1.0 / 3.0 + h2 * (1.0 / 45.0 + h2 * (2.0 / 945.0 + h2 * (1.0 / 4725.0 + h2 * (2.0 / 93555.0)))));
        *da_dw = -h * (1.0 / 3.0 + h2 * (2.0 / 45.0 + h2 * (2.0 / 315.0 + h2 * (4.0 / 4725.0 + h2 * (2.0 / 18711.0)))));
        *dlogdet_dw = h * (1.0 / 3.0 + h2 * (1.0 / 45.0 + h2 * (2.0 / 945.0 + h2 * (1.0 / 4725.0 + h2 * (2.0 / 93555.0)))));
    } else {
        double sh, ch;
        sincos(h, &sh, &ch);
        const double cot = ch / sh;
        *a = h * cot;
        *da_dw = 0.5 * (cot - h / (sh * sh));
        *dlogdet_dw = 1.0 / h - cot;
    }
}

// d/d(tx, ty, w) of se2_tangent_log_pdf: v = (a tx + h ty, a ty - h tx, w), L = c - v'Pv / 2 + logdet(w)
__device__ __forceinline__ void se2_tangent_score(double tx, double ty, double w, const double* __restrict__ p, double* gtx,
                                                  double* gty, double* gw) {
    double a, da, dl;
    log_map_terms(w, &a, &da, &dl);
    const double h = 0.5 * w;
    const double vx = a * tx + h * ty, vy = a * ty - h * tx;
    const double gvx = -(p[3] * vx + p[4] * vy + p[5] * w);
    const double gvy = -(p[4] * vx + p[6] * vy + p[7] * w);
    const double gvw = -(p[5] * vx + p[7] * vy + p[8] * w);
    *gtx = a * gvx - h * gvy;
    *gty = h * gvx + a * gvy;
    *gw = gvw + gvx * (da * tx + 0.5 * ty) + gvy * (da * ty - 0.5 * tx) + dl;
}

// The second derivatives in w: a''(w) = (a - 1) / (2 sin^2 h) and l''(w) = (1 / sin^2 h - 1 / h^2) / 2.  Both are differences
// of two terms of size 1 / h^2 that leave -1/6 resp. 1/6: the plain forms lose 3 eps / h^2 resp. 6 eps / h^2 relative, twice
// and four times what a' and l' lose, so at SERIES_H = 0.1 they would have lost 300 and 600 roundings, and l'' is the whole
// heading-heading entry of a loose prior.  The series (the derivatives of the series above, coefficients 2^2k |B_2k| / (2k)!
// times 2k (2k - 1) / 4 resp. (2k - 1) / 2) converge like (h / pi)^2k, so the switch moves OUT and the series grow: through
// h^16, below SERIES2_H = 0.3.  There the plain forms have lost 3 eps / h^2 = 33 and 6 eps / h^2 = 67 roundings, and the first
// dropped terms, 2.2e-8 h^18 and 2.2e-9 h^18 against 1/6, are 5e-17 and 5e-18 relative (under half a rounding): the plain side
// is the worse one at the switch and only improves beyond it, and a switch further out (h = 0.5: 12 and 24 roundings) would
// need the series through h^22 for the same balance.
constexpr double SERIES2_H = 0.3;

__device__ __forceinline__ void log_map_curvature(double w, double a, double* dda_dw, double* ddlogdet_dw) {
    const double h = 0.5 * w;
    if (fabs(h) < SERIES2_H) {
        const double h2 = h * h;
        *dda_dw = -(1.0 / 6.0 + h2 * (1.0 / 15.0 + h2 * (1.0 / 63.0 + h2 * (2.0 / 675.0 + h2 * (1.0 / 2079.0 + h2 * (1382.0 / 19348875.0 +
                  h2 * (2.0 / 200475.0 + h2 * (14468.0 / 10854718875.0 + h2 * (43867.0 / 254766637125.0)))))))));
        *ddlogdet_dw = 1.0 / 6.0 + h2 * (1.0 / 30.0 + h2 * (1.0 / 189.0 + h2 * (1.0 / 1350.0 + h2 * (1.0 / 10395.0 + h2 * (691.0 / 58046625.0 +
                       h2 * (2.0 / 1403325.0 + h2 * (3617.0 / 21709437750.0 + h2 * (43867.0 / 2292899734125.0))))))));
    } else {
        const double sh = sin(h);
        const double is2 = 1.0 / (sh * sh);
        *dda_dw = 0.5 * (a - 1.0) * is2;
        *ddlogdet_dw = 0.5 * (is2 - 1.0 / (h * h));
    }
}

// The gradient (gtx, gty: what the chain rule of a relative pose needs again) and the Hessian-vector product of
// se2_tangent_log_pdf along (vtx, vty, vw): the derivative of se2_tangent_score along that direction, term by term.  With
// v = (a tx + h ty, a ty - h tx, w), j = dv/dw = (a' tx + ty / 2, a' ty - tx / 2), gv = -P v:
//   dv = A (vtx, vty) + j vw,   dgv = -P (dv, vw),   d gt = A' dgv_xy + A'(w)' gv_xy vw,
//   d gw = dgv_w + dgv_xy . j + gv_xy . (a'' vw t + A'(w) (vtx, vty)) + l'' vw
__device__ __forceinline__ void se2_tangent_hvp(double tx, double ty, double w, const double* __restrict__ p, double vtx,
                                                double vty, double vw, double* gtx, double* gty, double* htx, double* hty,
                                                double* hw) {
    double a, da, dl, dda, ddl;
    log_map_terms(w, &a, &da, &dl);
    log_map_curvature(w, a, &dda, &ddl);
    const double h = 0.5 * w;
    const double vx = a * tx + h * ty, vy = a * ty - h * tx;
    const double gvx = -(p[3] * vx + p[4] * vy + p[5] * w);
    const double gvy = -(p[4] * vx + p[6] * vy + p[7] * w);
    *gtx = a * gvx - h * gvy;
    *gty = h * gvx + a * gvy;
    const double jx = da * tx + 0.5 * ty, jy = da * ty - 0.5 * tx;
    const double dvx = a * vtx + h * vty + jx * vw, dvy = a * vty - h * vtx + jy * vw;
    const double dgvx = -(p[3] * dvx + p[4] * dvy + p[5] * vw);
    const double dgvy = -(p[4] * dvx + p[6] * dvy + p[7] * vw);
    const double dgvw = -(p[5] * dvx + p[7] * dvy + p[8] * vw);
    *htx = a * dgvx - h * dgvy + (da * gvx - 0.5 * gvy) * vw;
    *hty = h * dgvx + a * dgvy + (0.5 * gvx + da * gvy) * vw;
    *hw = dgvw + dgvx * jx + dgvy * jy + gvx * (dda * vw * tx + da * vtx + 0.5 * vty) + gvy * (dda * vw * ty + da * vty - 0.5 * vtx) +
          ddl * vw;
}

// ---- the range term log N(|a - b| - d; 0, 1 / inv_var), and its d/da (d/db is the negative): the zero vector at |a - b| = 0,
// where the range has no direction
__device__ __forceinline__ double range_log_pdf(double ax, double ay, double bx, double by, double d, double inv_var,
                                                double log_norm) {
    const double dx = ax - bx, dy = ay - by;
    const double delta = sqrt(dx * dx + dy * dy) - d;
    return log_norm - 0.5 * delta * delta * inv_var;
}
__device__ __forceinline__ void range_score(double ax, double ay, double bx, double by, double d, double inv_var, double* gx,
                                            double* gy) {
    const double dx = ax - bx, dy = ay - by;
    const double r = sqrt(dx * dx + dy * dy);
    const double c = (r > 0.0) ? -(r - d) * inv_var / r : 0.0;
    *gx = c * dx, *gy = c * dy;
}

// The a-a block of the range term's Hessian times q: with r = |a - b|, u = (a - b) / r, delta = r - d it is
// -inv_var [u u' + (delta / r) (I - u u')] q  (the b-b block is the same, the a-b block its negative: q = v_a - v_b gives the
// rows of a, the negative those of b); the zero vector at r = 0, like the score.
__device__ __forceinline__ void range_hvp(double ax, double ay, double bx, double by, double d, double inv_var, double qx,
                                          double qy, double* hx, double* hy) {
    const double dx = ax - bx, dy = ay - by;
    const double r = sqrt(dx * dx + dy * dy);
    *hx = 0.0, *hy = 0.0;
    if (r > 0.0) {
        const double ux = dx / r, uy = dy / r;
        const double uq = ux * qx + uy * qy, k = (r - d) / r;
        *hx = -inv_var * (ux * uq + k * (qx - ux * uq));
        *hy = -inv_var * (uy * uq + k * (qy - uy * uq));
    }
}

// ---- the R2 Gaussian of the residual (dx, dy), and its d/d(dx, dy): p[2..4] = upper triangle of the precision, p[5] = log norm
__device__ __forceinline__ double r2_log_pdf(double dx, double dy, const double* __restrict__ p) {
    return p[5] - 0.5 * (p[2] * dx * dx + p[4] * dy * dy + 2.0 * p[3] * dx * dy);
}
__device__ __forceinline__ void r2_score(double dx, double dy, const double* __restrict__ p, double* gx, double* gy) {
    *gx = -(p[2] * dx + p[3] * dy), *gy = -(p[3] * dx + p[4] * dy);
}

}  // namespace factor_model
