// factor_score.hip — the score of the factor graph's joint density, G[r][p] = d/dx_r log p(X, Z) at point p.
//
// The reference has `grad_x_log_pdf` on every factor class (src/factors/Factors.py:829-850, :1450-1478, :2203-2223,
// :2732-2751, :3135-3156) and adds them per variable in JointFactor.grad_x_log_pdf (src/sampler/sampler_utils.py:100-113),
// sample by sample in Python; its one consumer is the kernel Stein discrepancy (src/utils/Statistics.py:193-245).  Here the
// factors are the table of factor_density.hip (nfisam_factor_term, the same seven codes) and the points are the column-major
// float32 matrix St[total_dim][n]; the result is the float64 column-major matrix Gt[total_dim][n].
//
// Numerics: the contract of sample_common.h -- float32 points in, every operation float64: the derivative of the float64
// formula that factor_term() of factor_density.hip evaluates, at the float32 point.  It is the derivative of the SMOOTH
// formula everywhere: the value's own branches (|w| < 1e-10 in the log map, |w| < 1e-5 in its Jacobian) are flat spots of
// 1e-10 and get no derivative-zero plateaus.  A range of exactly 0 has no direction: its derivative is the zero vector.  A
// mixture's derivative is sum_j r_j grad term_j with r the softmax of the component terms, shifted by their maximum like the
// value's log-sum-exp: finite wherever the terms are.
//
// Two launches, no float atomics.  (1) like factor_terms_kernel: a wave owns a 64-point tile and a run of FAC_RUN factors,
// code and parameters wave-uniform; factor f writes its partial derivatives into its own slots slot_off[f] .. of the scratch
// [n_slots][n] (3 / 6 / 4 / 2 + 2k / 2 / 2 / 4 slots by code, in the order of the factor's rows: a, then b or the candidates).
// (2) a wave per (64-point tile, row r of G) adds the slots row_slot[row_off[r] .. row_off[r + 1]) in that order -- the host
// lists a row's slots in table order -- one accumulator per point.  A row without a slot is 0.  Hence: two calls give the same
// bits, and a point's column does not depend on n or on its tile.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nfisam_hip.h"
#include "sample_common.h"

namespace {

using namespace sample_common;

constexpr int FAC_RUN = 8;        // factors per wave in the first pass
constexpr int MAX_SLOTS = 10;     // a mixture of four: 2 + 2 * 4
constexpr int ADD_ROWS = 8;       // second pass: loads in flight per point

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

// d/d(tx, ty, w) of se2_tangent_log_pdf (factor_density.hip): v = (a tx + h ty, a ty - h tx, w), L = c - v'Pv / 2 + logdet(w)
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

// d/da of the range term -(|a - b| - d)^2 inv_var / 2 (d/db is its negative); the zero vector at |a - b| = 0
__device__ __forceinline__ void range_score(double ax, double ay, double bx, double by, double d, double inv_var, double* gx,
                                            double* gy) {
    const double dx = ax - bx, dy = ay - by;
    const double r = sqrt(dx * dx + dy * dy);
    const double c = (r > 0.0) ? -(r - d) * inv_var / r : 0.0;
    *gx = c * dx, *gy = c * dy;
}

__device__ __forceinline__ int slot_count(int code, int k) {
    switch (code) {
    case NFISAM_FAC_PRIOR_SE2: return 3;
    case NFISAM_FAC_REL_SE2: return 6;
    case NFISAM_FAC_RANGE: return 4;
    case NFISAM_FAC_RANGE_MIX: return (k >= 1 && k <= 4) ? 2 + 2 * k : 0;
    case NFISAM_FAC_PRIOR_R2: return 2;
    case NFISAM_FAC_PRIOR_R2_RANGE: return 2;
    case NFISAM_FAC_REL_R2: return 4;
    default: return 0;
    }
}

// one factor at one point: g[0 .. slot_count) in the order of its rows (a's, then b's or the candidates'); `t` is wave-uniform.
// The row checks are those of factor_term(): a bad record yields NaN in every slot and reads nothing.
__device__ __forceinline__ void factor_score(const nfisam_factor_term* __restrict__ t, const float* __restrict__ St, size_t n,
                                             size_t pp, int total_dim, double (&g)[MAX_SLOTS]) {
    const int code = t->code;
    const double* __restrict__ p = t->p;
#pragma unroll
    for (int s = 0; s < MAX_SLOTS; ++s) g[s] = NAN;
    const bool pose_a = code == NFISAM_FAC_PRIOR_SE2 || code == NFISAM_FAC_REL_SE2;
    const bool has_b = code == NFISAM_FAC_REL_SE2 || code == NFISAM_FAC_RANGE || code == NFISAM_FAC_REL_R2;
    if (code < NFISAM_FAC_PRIOR_SE2 || code > NFISAM_FAC_REL_R2) return;
    if (t->a < 0 || t->a + (pose_a ? 3 : 2) > total_dim) return;
    if (has_b && (t->b < 0 || t->b + (code == NFISAM_FAC_REL_SE2 ? 3 : 2) > total_dim)) return;
    const float* __restrict__ A = St + (size_t)t->a * n + pp;
    const double ax = (double)A[0], ay = (double)A[n];
    switch (code) {
    case NFISAM_FAC_PRIOR_SE2: {
        double s, c, gtx, gty, gw;
        sincos(p[2], &s, &c);
        const double dx = ax - p[0], dy = ay - p[1];
        const double w = wrap_pi(wrap_pi(-p[2]) + wrap_pi((double)A[2 * n]));
        se2_tangent_score(c * dx + s * dy, c * dy - s * dx, w, p, &gtx, &gty, &gw);
        g[0] = c * gtx - s * gty, g[1] = s * gtx + c * gty, g[2] = gw;
        return;
    }
    case NFISAM_FAC_REL_SE2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        const double thi = (double)A[2 * n], thj = (double)Bv[2 * n];
        double si, ci, so, co, gtx, gty, gw;
        sincos(thi, &si, &ci);
        sincos(p[2], &so, &co);
        const double dx = (double)Bv[0] - ax, dy = (double)Bv[n] - ay;
        const double ux = ci * dx + si * dy, uy = ci * dy - si * dx;          // the difference in pose i's frame
        const double rx = ux - p[0], ry = uy - p[1];
        const double w = wrap_pi(wrap_pi(-p[2]) + wrap_pi(wrap_pi(-wrap_pi(thi)) + wrap_pi(thj)));
        se2_tangent_score(co * rx + so * ry, co * ry - so * rx, w, p, &gtx, &gty, &gw);
        const double grx = co * gtx - so * gty, gry = so * gtx + co * gty;
        const double gx = ci * grx - si * gry, gy = si * grx + ci * gry;      // d/d(x_j, y_j)
        g[0] = -gx, g[1] = -gy, g[2] = grx * uy - gry * ux - gw;            // d ux / d th_i = uy, d uy / d th_i = -ux
        g[3] = gx, g[4] = gy, g[5] = gw;
        return;
    }
    case NFISAM_FAC_RANGE: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        double gx, gy;
        range_score(ax, ay, (double)Bv[0], (double)Bv[n], p[0], p[1], &gx, &gy);
        g[0] = gx, g[1] = gy, g[2] = -gx, g[3] = -gy;
        return;
    }
    case NFISAM_FAC_RANGE_MIX: {
        const int k = t->k;
        if (k < 1 || k > 4) return;
        for (int j = 0; j < k; ++j)
            if (t->cand[j] < 0 || t->cand[j] + 2 > total_dim) return;
        double term[4], gx[4], gy[4];
        double top = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            term[j] = -INFINITY, gx[j] = 0.0, gy[j] = 0.0;
            if (j < k) {
                const float* __restrict__ Cv = St + (size_t)t->cand[j] * n + pp;
                const double cx = (double)Cv[0], cy = (double)Cv[n];
                const double ddx = ax - cx, ddy = ay - cy;
                const double delta = sqrt(ddx * ddx + ddy * ddy) - p[3 * j];
                term[j] = p[3 * j + 2] - 0.5 * delta * delta * p[3 * j + 1];           // range_log_pdf of factor_density.hip
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
    case NFISAM_FAC_PRIOR_R2: {
        const double dx = ax - p[0], dy = ay - p[1];
        g[0] = -(p[2] * dx + p[3] * dy), g[1] = -(p[3] * dx + p[4] * dy);
        return;
    }
    case NFISAM_FAC_PRIOR_R2_RANGE: {
        double gx, gy;
        range_score(ax, ay, p[0], p[1], p[2], p[3], &gx, &gy);
        g[0] = gx, g[1] = gy;
        return;
    }
    case NFISAM_FAC_REL_R2: {
        const float* __restrict__ Bv = St + (size_t)t->b * n + pp;
        const double dx = (double)Bv[0] - ax - p[0], dy = (double)Bv[n] - ay - p[1];
        const double gx = -(p[2] * dx + p[3] * dy), gy = -(p[3] * dx + p[4] * dy);   // d/db
        g[0] = -gx, g[1] = -gy, g[2] = gx, g[3] = gy;
        return;
    }
    default:
        return;
    }
}

// grid (tiles of 64 points, runs of FAC_RUN factors), one wave per block
__global__ void __launch_bounds__(64) factor_score_kernel(const nfisam_factor_term* __restrict__ terms, int n_terms,
                                                          const float* __restrict__ St, int total_dim, int n,
                                                          const int32_t* __restrict__ slot_off, int n_slots,
                                                          double* __restrict__ slots) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    const size_t pp = (p < n) ? (size_t)p : (size_t)(n - 1);
    const int f0 = blockIdx.y * FAC_RUN;
    const int f1 = min(f0 + FAC_RUN, n_terms);
    for (int f = f0; f < f1; ++f) {
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
    if ((n_terms + FAC_RUN - 1) / FAC_RUN > 65535 || total_dim > 65535) return NFISAM_ERR_ARG;   // the grids' second dimension
    if ((long long)n_slots > (long long)MAX_SLOTS * n_terms) return NFISAM_ERR_ARG;
    if (n == 0) return NFISAM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n_terms == 0)                                                  // the empty graph: a zero score
        return launch_status(hipMemsetAsync(Gt, 0, (size_t)total_dim * n * sizeof(double), s));
    const int tiles = (n + 63) / 64;
    hipLaunchKernelGGL(factor_score_kernel, dim3(tiles, (n_terms + FAC_RUN - 1) / FAC_RUN), dim3(64), 0, s, terms, n_terms, St,
                       total_dim, n, slot_off, n_slots, scratch);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(score_gather_kernel, dim3(tiles, total_dim), dim3(64), 0, s, scratch, n_slots, n, row_off, row_slot, Gt);
        e = hipGetLastError();
    }
    return launch_status(e);
}
