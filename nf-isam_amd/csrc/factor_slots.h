// factor_slots.h -- what the slot evaluators of the factor graph (factor_score.hip: the gradient; factor_hessian.hip: the
// Hessian-vector product) share: a factor's partial derivatives in its own slots (factor_score(), one slot per row the
// factor reads), and the ordered gather that adds the slots of a row (score_gather_kernel, with its launch).  Each unit that
// includes this header gets its own copy of the kernel (internal linkage): one text, no second version of it.
#pragma once
#include "factor_model.h"

namespace factor_model {
namespace {

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


// the gather's launch: Out[r][p] = the ordered sum of row r's slots, for every row of [total_dim][n]
inline hipError_t launch_gather(const double* slots, int n_slots, int n, int total_dim, const int32_t* row_off,
                                const int32_t* row_slot, double* Out, hipStream_t s) {
    hipLaunchKernelGGL(score_gather_kernel, dim3((n + 63) / 64, total_dim), dim3(64), 0, s, slots, n_slots, n, row_off, row_slot, Out);
    return hipGetLastError();
}

}  // namespace
}  // namespace factor_model
