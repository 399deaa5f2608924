#!/usr/bin/env python3
"""The factor densities and their gradients to 60 digits, written from the mathematics (python + mpmath, `mp.dps = 60`; no GPU,
no reference checkout, nothing of this project's own formulas: neither factors/Factors.py nor csrc/factor_model.h is read).

Writes tests/golden/factor_exact.npz, the yardstick of `Factors.*.log_pdf` / `grad_x_log_pdf` and of the device entries
`nfisam_factor_graph_log_density` / `nfisam_factor_graph_score` (tests/test_factor_exact_cpu.py, tests/test_factor_exact_gpu.py).

What is evaluated.  Every factor is built from its CONSTRUCTOR parameters (observation, covariance, range, sigma, weights) --
the packed table row is never used, so the precision triangle, the log normaliser and the log weights are graded too -- at
float32 points, as the SMOOTH density with no small-angle branch:
    SE(2) prior / relative pose   log N(Log(dT); 0, Sigma) + log|det dLog|,  dT = obs^-1 T  resp.  obs^-1 (T_i^-1 T_j),
                                  Log(t, w) = (V(w)^-1 t, w),  V(w) = [[sin w, cos w - 1], [1 - cos w, sin w]] / w,
                                  |det dLog| = w^2 / (2 - 2 cos w); the heading residual w reduced to [-pi, pi) exactly
    range / ring prior            log N(|a - b| - d; 0, sigma^2)
    mixtures                      log sum_j w_j N(|a - c_j| - d_j; 0, sigma_j^2), w normalised exactly
    R2 Gaussian prior / relative  the bivariate normal of x - mu  resp.  b - a - observation
Two evaluations are made of every value and must agree to 1e-25 of the value's scale (asserted for every case point and for
every seventh graph term):
  * `plain_log_pdf`: the definition, in homogeneous 3 x 3 pose matrices, `atan2`, a linear solve with V(w) and the plain
    log of a sum of exponentials; its gradient by `mpmath.diff`;
  * `evaluate`: the same density and its analytic gradient (derived below, next to each formula) in the half-angle form, in
    an arithmetic that carries a running error bound with every value (class R).
What is stored, per value, as float64 rounded from 60 digits (scales rounded up; the graphs' scales as float32):
    exact   the value;
    scale   the running bound: the same expression with every difference replaced by the sum of the absolute values,
            carried from the inputs on.  Inputs are exact; the result of an operation is no smaller than its own magnitude;
            a sum or difference adds the bounds of its operands; a product or quotient takes the larger of the two
            operands' relative bounds; a function f(u) takes max(|f|, |f'(u)| bound(u)); no bound of a computed value is
            below 2^-968 (float64 underflows: a mixture weight of 1e-300 times exp(-50)).  The heading residual enters with
            |th| + |p2| + pi (a relative pose: |th_i| + |th_j| + |p2| + pi): every wrap of a heading rounds against pi.
            So the rotated offsets get |c dx| + |s dy|, the quadratic form the sum of the magnitudes of its summands, a
            determinant the sum of the magnitudes of its products.  The log-map terms a(w) = (w/2) cot(w/2), a'(w),
            l(w) = log|det dLog| and l'(w) count as functions of w.  An evaluation in float64 may differ from `exact` by
            C x 2^-53 x scale, C counting the roundings along the longest chain (the tests: C = 256);
    allow   the documented flat spot of the VALUE's own branches: w^2 / 12 where |w| < 1e-5 (the value takes |det dLog| = 1
            there), 0 otherwise.  The score gets none: csrc/factor_score.hip promises the smooth derivative everywhere;
    mask    (the score only) False at a range of exactly 0, where the score has no direction; the stored score is 0 there.

The cases (at most 64 points each; `<name>_cls`, `<name>_params` [m or 1, p], `<name>_x` float32 [m, width]; row i of x belongs
to row i of params, or to the one row there is).  Parameter layouts are those of tests/golden/make_factor_density_fixture.py,
except AmbiguousDataAssociationFactor: k, weights(k), observation, sigma, landmark index of every component (k).
  * a000 .. a027: every part-(a) case of tests/golden/factor_density.npz, its parameters and points read from that file
    (neither is stored again);
  * se2_prior_* / se2_rel_* with a tight diag(1e-8, 1e-10, 1e-12), a medium and a full random covariance: one observation per
    point, its heading chosen in double so that w lands on +-{0, 1e-12, 9.9e-11, 1.01e-10, 1e-8, 9.9e-6, 1.01e-5, 1e-4, 1e-3,
    0.05, nextafter(0.2, 0), 0.2, 0.21, 1, 3, pi - 1e-3, pi - 1e-5}, with headings that are other representatives (+-3.5,
    2 pi + 0.1, +-float32(pi), up to 3 pi) and poses up to 1e4 m from the origin;
  * se2_prior_loose: covariance diag(1, 1, 9), 48 residuals between 2e-3 and 0.2 (half of them in [2e-3, 4e-3]): where l'(w)
    dominates the heading's score and a displaced small-angle switch would show;
  * range_*, ring_*: separations of 0 (masked), one float32 denormal, 1e19 per coordinate; a measured range of 0;
  * mix_*: k = 1 .. 4, tied components, one component ahead by 1e4 in the log, every component 1e4 m away, a candidate
    listed twice (and the null-hypothesis factor), a weight of 1e-300 before normalisation;
  * r2_*: correlation 0.999999, points 1e4 sigma out;
  * whole graphs: tests/data/ManhattanPlaza136 and Plaza1ADA0.4EFG at rows that tests/golden/factor_score.npz names (every
    sixth / every second of them: the file stays below that fixture's size) and the first 64 points of its 13-dimensional
    KSD graph: per-factor terms, the total and the joint score, with their scales and allowances.

What the script asserts of its own output (caps, fixed before anything was measured against them):
  * no point within 1e-6 of the heading wrap |w| = pi (the density jumps there; a rounding must not pick the side);
  * masked rows: at most 5 % of a case, and only at a range of exactly 0;
  * 256 x 2^-53 x scale <= 1e-9 (|exact| + 1) on at least 90 % of the values and of the scores of every case that `exempt`
    does not name.  `exempt` is written down here, case by case with the reason, not computed;
  * 256 x 2^-53 x scale <= (|exact| + 1) / 4 on EVERY value: a wrong sign of anything of size 1/7 or more shows everywhere.

    python tests/golden/make_factor_exact_fixture.py
"""
import os
import sys

import mpmath
import numpy as np
from mpmath import mp, mpf

mp.dps = 60

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "factor_exact.npz")
DENSITY = os.path.join(HERE, "factor_density.npz")
SCORE = os.path.join(HERE, "factor_score.npz")
DATA = os.path.join(os.path.dirname(HERE), "data")
GRAPHS = {"manhattan136": ("ManhattanPlaza136", slice(0, None, 6)), "plaza1ada": ("Plaza1ADA0.4EFG", slice(0, None, 2))}
KSD_POINTS = 64
C_BOUND, CAP, VACUOUS = 256, 1e-9, 0.25
EPS = 2.0 ** -53
SE2 = ("UnarySE2ApproximateGaussianPriorFactor", "SE2RelativeGaussianLikelihoodFactor")
# the cases that miss the 1e-9 cap, and why: the bound is honest there, not loose
EXEMPT = {
    "a000": "prior with covariance diag(1e-8, 1e-10, 1e-12): the precision 1e12 multiplies the heading's rounding against pi",
    "a001": "prior with covariance diag(1e-4, 1e-6, 1e-8), heading next to +pi: the same, precision 1e8",
    "se2_prior_tight": "covariance diag(1e-8, 1e-10, 1e-12)",
    "se2_rel_tight": "covariance diag(1e-8, 1e-10, 1e-12), offsets of metres against residuals of 1e-4 m",
    "r2_prior_corr": "correlation 0.999999: the determinant 1 - rho^2 cancels six digits",
    "r2_rel_corr": "correlation 0.999999, and b - a - observation cancels at 1e4 m",
}


# float64 underflows: a softmax weight of 1e-300 times exp(-50) is a denormal or 0.  No computed value's bound is below TINY, so
# that a bound times 2^-53 is still a normal number (2^-1021) and nothing smaller than 1e-291 is ever asked for
TINY = mpf(2) ** -968


# ---- values with a running bound ------------------------------------------------------------------------------------------------
class R(object):
    """A 60-digit value `v` and the running bound `e` of the module docstring (in units of the rounding unit)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v, self.e = mpf(v), mpf(e)

    @staticmethod
    def of(a):
        return a if isinstance(a, R) else R(a)

    @staticmethod
    def made(v, carried):
        if v == 0 and carried == 0:
            return R(0)                              # a structural zero stays exact
        return R(v, max(carried, abs(v), TINY))

    def __add__(self, o):
        o = R.of(o)
        return R.made(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = R.of(o)
        return R.made(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return R.of(o) - self

    def __neg__(self):
        return R(-self.v, self.e)

    def __mul__(self, o):
        o = R.of(o)
        return R.made(self.v * o.v, max(self.e * abs(o.v), abs(self.v) * o.e))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R.of(o)
        q = self.v / o.v
        return R.made(q, max(self.e / abs(o.v), abs(q) * o.e / abs(o.v)))

    def fun(self, f, df):
        """f(self) with derivative df."""
        return R.made(f, abs(df) * self.e)


def r_sin(a):
    return a.fun(mp.sin(a.v), mp.cos(a.v))


def r_cos(a):
    return a.fun(mp.cos(a.v), mp.sin(a.v))


def r_log(a):
    return a.fun(mp.log(a.v), 1 / a.v)


def r_exp(a):
    return a.fun(mp.exp(a.v), mp.exp(a.v))


def r_sqrt(a):
    s = mp.sqrt(a.v)
    return a.fun(s, 1 / (2 * s)) if s != 0 else R(0)


def total(items):
    acc = R(0)
    for it in items:
        acc = acc + it
    return acc


def gaussian_parts(cov):
    """covariance (exact floats, n = 2 or 3) -> (precision [n][n] of R by cofactors, log normaliser R)."""
    n = len(cov)
    c = [[R(float(cov[i][j])) for j in range(n)] for i in range(n)]
    if n == 2:
        cof = [[c[1][1], -c[1][0]], [-c[0][1], c[0][0]]]
    else:
        cof = [[c[(i + 1) % 3][(j + 1) % 3] * c[(i + 2) % 3][(j + 2) % 3] - c[(i + 1) % 3][(j + 2) % 3] * c[(i + 2) % 3][(j + 1) % 3]
                for j in range(3)] for i in range(3)]
    det = total(c[0][j] * cof[0][j] for j in range(n))
    inv = [[cof[j][i] / det for j in range(n)] for i in range(n)]
    # v' S^-1 v only sees the symmetric part (a covariance given as Q D Q' in floating point is symmetric to a rounding only)
    prec = [[inv[i][j] if i == j else (inv[i][j] + inv[j][i]) * 0.5 for j in range(n)] for i in range(n)]
    return prec, -(n * r_log(R(2 * mp.pi)) + r_log(det)) * 0.5


def quad(prec, v):
    """(P v, v' P v): every summand enters the bound with its magnitude."""
    pv = [total(prec[i][j] * v[j] for j in range(len(v))) for i in range(len(v))]
    return pv, total(v[i] * pv[i] for i in range(len(v)))


def reduce_heading(t):
    """t -> the representative in [-pi, pi)."""
    return t - 2 * mp.pi * mp.floor((t + mp.pi) / (2 * mp.pi))


def log_map_terms(w):
    """a = h cot h with h = w / 2, a' = da / dw, l = log(w^2 / (4 sin^2 h)), l' = dl / dw as functions of the R value w:
         a' = (cot h - h / sin^2 h) / 2,   a'' = (a - 1) / (2 sin^2 h),   l' = 1 / h - cot h,   l'' = (1 / sin^2 h - 1 / h^2) / 2
    and at w = 0 their limits 1, 0, -1/6; 0, 0, 1/6 (the one removable point, no branch)."""
    x = w.v
    if x == 0:
        a, da, dda, ln, dl, ddl = mpf(1), mpf(0), -mpf(1) / 6, mpf(0), mpf(0), mpf(1) / 6
    else:
        h = x / 2
        cot, s2 = mp.cot(h), 1 / mp.sin(h) ** 2
        a = h * cot
        da, dda = (cot - h * s2) / 2, (a - 1) * s2 / 2
        ln, dl, ddl = 2 * mp.log(abs(h / mp.sin(h))), 1 / h - cot, (s2 - 1 / h ** 2) / 2
    ln_r = w.fun(ln, dl)
    ln_r.e = max(ln_r.e, mpf(2))                 # twice the log of a quotient next to 1: two rounding units, absolutely
    return w.fun(a, da), w.fun(da, dda), ln_r, w.fun(dl, ddl)


def se2_tangent(tx, ty, w, cov):
    """L(t, w) = log N((A t, w); 0, Sigma) + l(w), A = [[a, h], [-h, a]] (= V(w)^-1), and its gradient:
         dL/dt = -A' (P v)_xy,    dL/dw = -(P v) . (A'(w) t, 1) + l'(w),   A'(w) = [[a', 1/2], [-1/2, a']]."""
    prec, log_norm = gaussian_parts(cov)
    a, da, ln, dl = log_map_terms(w)
    h = w * 0.5
    v = [a * tx + h * ty, a * ty - h * tx, w]
    pv, q = quad(prec, v)
    value = log_norm - q * 0.5 + ln
    gtx = -(a * pv[0] - h * pv[1])
    gty = -(h * pv[0] + a * pv[1])
    gw = dl - (pv[0] * (da * tx + ty * 0.5) + pv[1] * (da * ty - tx * 0.5) + pv[2])
    return value, gtx, gty, gw


def flat_spot(w):
    return w * w / 12 if abs(w) < mpf("1e-5") else mpf(0)


def eval_se2_prior(p, x):
    px, py, pth = (R(float(t)) for t in p[:3])
    cov = np.asarray(p[3:12], dtype=np.float64).reshape(3, 3)
    c, s = r_cos(pth), r_sin(pth)
    dx, dy = R(x[0]) - px, R(x[1]) - py
    tx, ty = c * dx + s * dy, c * dy - s * dx
    wv = reduce_heading(mpf(x[2]) - pth.v)
    w = R(wv, abs(mpf(x[2])) + abs(pth.v) + mp.pi)
    value, gtx, gty, gw = se2_tangent(tx, ty, w, cov)
    # t = R(pth)' (xy - p): d t / d xy = R(pth)', so the gradient goes back through R(pth)
    return value, [c * gtx - s * gty, s * gtx + c * gty, gw], wv, True


def eval_se2_relative(p, x):
    ox, oy, oth = (R(float(t)) for t in p[:3])
    cov = np.asarray(p[3:12], dtype=np.float64).reshape(3, 3)
    thi, thj = R(x[2]), R(x[5])
    ci, si, co, so = r_cos(thi), r_sin(thi), r_cos(oth), r_sin(oth)
    dx, dy = R(x[3]) - R(x[0]), R(x[4]) - R(x[1])
    ux, uy = ci * dx + si * dy, ci * dy - si * dx               # u = R(th_i)' (t_j - t_i)
    rx, ry = ux - ox, uy - oy
    tx, ty = co * rx + so * ry, co * ry - so * rx               # t = R(oth)' (u - o)
    wv = reduce_heading(thj.v - thi.v - oth.v)
    w = R(wv, abs(thi.v) + abs(thj.v) + abs(oth.v) + mp.pi)
    value, gtx, gty, gw = se2_tangent(tx, ty, w, cov)
    grx, gry = co * gtx - so * gty, so * gtx + co * gty         # d/du
    gbx, gby = ci * grx - si * gry, si * grx + ci * gry         # d/dt_j = R(th_i) d/du; d/dt_i is its negative
    # du/dth_i = (uy, -ux), dw/dth_i = -1, dw/dth_j = 1
    return value, [-gbx, -gby, grx * uy - gry * ux - gw, gbx, gby, gw], wv, True


def range_term(ax, ay, bx, by, d, sigma):
    """log N(|a - b| - d; 0, sigma^2) and its gradient in a (in b: the negative); (None, None) for the gradient at |a - b| = 0."""
    dx, dy = R(ax) - R(bx), R(ay) - R(by)
    r = r_sqrt(dx * dx + dy * dy)
    var = R(float(sigma)) * R(float(sigma))
    delta = r - R(float(d))
    value = -(r_log(R(2 * mp.pi) * var)) * 0.5 - delta * delta / var * 0.5
    if r.v == 0:
        return value, None
    coef = -(delta / var) / r
    return value, (coef * dx, coef * dy)


def eval_range(p, x, pose):
    o = 3 if pose else 2
    value, g = range_term(x[0], x[1], x[o], x[o + 1], p[0], p[1])
    if g is None:
        return value, [R(0)] * (o + 2), None, False
    return value, [g[0], g[1]] + ([R(0)] if pose else []) + [-g[0], -g[1]], None, True


def eval_ring(p, x):
    value, g = range_term(x[0], x[1], p[0], p[1], p[2], p[3])
    if g is None:
        return value, [R(0), R(0)], None, False
    return value, [g[0], g[1]], None, True


def eval_mixture(weights, cands, ds, sigmas, x, n_landmarks):
    """log sum_j w_j N(|a - c_j| - d_j; 0, sigma_j^2) by log-sum-exp around the largest term, and its gradient with the
    softmax weights; cands[j] is the landmark of component j (repeats add into the same columns)."""
    wsum = total(R(float(t)) for t in weights)
    terms, grads, ok = [], [], True
    for wj, cj, dj, sj in zip(weights, cands, ds, sigmas):
        value, g = range_term(x[0], x[1], x[3 + 2 * cj], x[4 + 2 * cj], dj, sj)
        ok = ok and g is not None
        terms.append(value + r_log(R(float(wj)) / wsum))
        grads.append(g)
    top = max(range(len(terms)), key=lambda j: terms[j].v)
    es = [R(1) if j == top else r_exp(terms[j] - terms[top]) for j in range(len(terms))]
    acc = total(es)
    value = terms[top] + r_log(acc)
    out = [R(0)] * (3 + 2 * n_landmarks)
    if ok:
        for j, cj in enumerate(cands):
            rj = es[j] / acc
            gx, gy = rj * grads[j][0], rj * grads[j][1]
            out[0], out[1] = out[0] + gx, out[1] + gy
            out[3 + 2 * cj], out[4 + 2 * cj] = out[3 + 2 * cj] - gx, out[4 + 2 * cj] - gy
    return value, out, None, ok


def eval_r2(mu, cov, d):
    prec, log_norm = gaussian_parts(cov)
    res = [d[0] - R(float(mu[0])), d[1] - R(float(mu[1]))]
    pv, q = quad(prec, res)
    return log_norm - q * 0.5, [-pv[0], -pv[1]]


def evaluate(cls, p, x):
    """One factor of class `cls` with constructor parameters p at the float32 point x -> dict of mpf: logp, logp_scale,
    logp_allow, score, score_scale (lists), mask, w (None outside SE(2))."""
    p = [float(t) for t in p]
    x = [mpf(float(t)) for t in x]
    if cls == SE2[0]:
        value, grad, w, ok = eval_se2_prior(p, x)
    elif cls == SE2[1]:
        value, grad, w, ok = eval_se2_relative(p, x)
    elif cls == "SE2R2RangeGaussianLikelihoodFactor":
        value, grad, w, ok = eval_range(p, x, True)
    elif cls == "R2RangeGaussianLikelihoodFactor":
        value, grad, w, ok = eval_range(p, x, False)
    elif cls == "UnaryR2RangeGaussianPriorFactor":
        value, grad, w, ok = eval_ring(p, x)
    elif cls == "AmbiguousDataAssociationFactor":
        k = int(p[0])
        cands = [int(t) for t in p[3 + k:3 + 2 * k]] if len(p) > 3 + k else list(range(k))
        value, grad, w, ok = eval_mixture(p[1:1 + k], cands, [p[1 + k]] * k, [p[2 + k]] * k, x, max(cands) + 1)
    elif cls == "BinaryFactorWithNullHypo":
        value, grad, w, ok = eval_mixture(p[:2], [0, 0], [p[2]] * 2, [p[3], p[3] * p[4]], x, 1)
    elif cls == "UnaryR2GaussianPriorFactor":
        value, grad = eval_r2(p[:2], np.array(p[2:6]).reshape(2, 2), [R(x[0]), R(x[1])])
        w, ok = None, True
    elif cls == "R2RelativeGaussianLikelihoodFactor":
        value, g = eval_r2(p[:2], np.array(p[2:6]).reshape(2, 2), [R(x[2]) - R(x[0]), R(x[3]) - R(x[1])])
        grad, w, ok = [-g[0], -g[1], g[0], g[1]], None, True
    else:
        raise KeyError(cls)
    return dict(logp=value.v, logp_scale=value.e, logp_allow=flat_spot(w) if w is not None else mpf(0),
                score=[g.v if ok else mpf(0) for g in grad], score_scale=[g.e if ok else mpf(0) for g in grad], mask=ok, w=w)


# ---- the definition once more, plainly, for mpmath.diff ----------------------------------------------------------------------
def pose_matrix(x, y, th):
    return mp.matrix([[mp.cos(th), -mp.sin(th), x], [mp.sin(th), mp.cos(th), y], [0, 0, 1]])


def plain_normal(v, cov):
    s = mp.matrix([[mpf(float(t)) for t in row] for row in np.asarray(cov, dtype=np.float64)])
    u = mp.matrix(list(v))
    return -(len(v) * mp.log(2 * mp.pi) + mp.log(mp.det(s))) / 2 - (u.T * mp.inverse(s) * u)[0] / 2


def plain_se2(dT, cov):
    w, t = mp.atan2(dT[1, 0], dT[0, 0]), mp.matrix([dT[0, 2], dT[1, 2]])
    if w == 0:
        return plain_normal([t[0], t[1], w], cov)
    versine = 2 * mp.sin(w / 2) ** 2                                            # 1 - cos w, without the cancellation
    V = mp.matrix([[mp.sin(w), -versine], [versine, mp.sin(w)]]) / w
    v = mp.lu_solve(V, t)
    return plain_normal([v[0], v[1], w], cov) + mp.log(w * w / (2 * versine))


def plain_range(ax, ay, bx, by, d, sigma):
    d, sigma = mpf(float(d)), mpf(float(sigma))
    r = mp.sqrt((ax - bx) ** 2 + (ay - by) ** 2)
    return -mp.log(2 * mp.pi * sigma ** 2) / 2 - (r - d) ** 2 / (2 * sigma ** 2)


def plain_log_pdf(cls, p, x):
    p = [float(t) for t in p]
    if cls in SE2:
        obs = pose_matrix(*[mpf(t) for t in p[:3]])
        cov = np.array(p[3:12]).reshape(3, 3)
        if cls == SE2[0]:
            return plain_se2(mp.inverse(obs) * pose_matrix(*x[:3]), cov)
        return plain_se2(mp.inverse(obs) * mp.inverse(pose_matrix(*x[:3])) * pose_matrix(*x[3:6]), cov)
    if cls == "SE2R2RangeGaussianLikelihoodFactor":
        return plain_range(x[0], x[1], x[3], x[4], p[0], p[1])
    if cls == "R2RangeGaussianLikelihoodFactor":
        return plain_range(x[0], x[1], x[2], x[3], p[0], p[1])
    if cls == "UnaryR2RangeGaussianPriorFactor":
        return plain_range(x[0], x[1], mpf(p[0]), mpf(p[1]), p[2], p[3])
    if cls in ("AmbiguousDataAssociationFactor", "BinaryFactorWithNullHypo"):
        if cls == "BinaryFactorWithNullHypo":
            ws, cands, sig, d = p[:2], [0, 0], [p[3], p[3] * p[4]], p[2]
        else:
            k = int(p[0])
            ws, d, sig = p[1:1 + k], p[1 + k], [p[2 + k]] * k
            cands = [int(t) for t in p[3 + k:3 + 2 * k]] if len(p) > 3 + k else list(range(k))
        wsum = sum(mpf(t) for t in ws)
        return mp.log(sum(mpf(wj) / wsum * mp.exp(plain_range(x[0], x[1], x[3 + 2 * c], x[4 + 2 * c], d, s))
                          for wj, c, s in zip(ws, cands, sig)))
    if cls == "UnaryR2GaussianPriorFactor":
        return plain_normal([x[0] - mpf(p[0]), x[1] - mpf(p[1])], np.array(p[2:6]).reshape(2, 2))
    if cls == "R2RelativeGaussianLikelihoodFactor":
        return plain_normal([x[2] - x[0] - mpf(p[0]), x[3] - x[1] - mpf(p[1])], np.array(p[2:6]).reshape(2, 2))
    raise KeyError(cls)


def cross_check(cls, p, x, got, what):
    """`evaluate`'s value and gradient against the plain definition and its `mpmath.diff`: 1e-25 of the scale."""
    xs = tuple(mpf(float(t)) for t in x)
    plain = plain_log_pdf(cls, p, xs)
    assert abs(plain - got["logp"]) <= mpf("1e-25") * got["logp_scale"], (what, plain, got["logp"])
    if not got["mask"]:
        return
    for c in range(len(xs)):
        order = tuple(1 if j == c else 0 for j in range(len(xs)))
        d = mp.diff(lambda *a: plain_log_pdf(cls, p, a), xs, order)
        assert abs(d - got["score"][c]) <= mpf("1e-25") * (got["score_scale"][c] + 1), (what, c, d, got["score"][c])


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def spd(rng, d, lo, hi):
    q, _ = np.linalg.qr(rng.randn(d, d))
    m = (q * np.exp(rng.uniform(np.log(lo), np.log(hi), d))) @ q.T
    return 0.5 * (m + m.T)


def to_double(v):
    return float(mpf(v))


W_TARGETS = [0.0, 1e-12, 9.9e-11, 1.01e-10, 1e-8, 9.9e-6, 1.01e-5, 1e-4, 1e-3, 0.05, float(np.nextafter(0.2, 0.0)), 0.2, 0.21,
             1.0, 3.0, float(np.pi) - 1e-3, float(np.pi) - 1e-5]
REPRESENTATIVES = [3.5, -3.5, 2 * np.pi + 0.1, float(np.float32(np.pi)), -float(np.float32(np.pi)), 9.42, -9.42, 7.0]


def heading_plan(rng):
    """[(point heading th (float32), target w)]: every target with both signs, at a heading of 0 (the observation's heading is
    then -w exactly), at a small heading or at a random one up to 3 pi; then the other representatives with moderate w."""
    plan = []
    for i, t in enumerate(W_TARGETS):
        for sign in ((1.0,) if t == 0.0 else (1.0, -1.0)):
            th = (0.0, float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-3 * np.pi, 3 * np.pi)))[(i + (sign < 0)) % 3]
            plan.append((float(np.float32(th)), sign * t))
    for th in REPRESENTATIVES:
        plan.append((float(np.float32(th)), float(rng.uniform(-2.5, 2.5))))
    return plan


def se2_cases(rng):
    covs = {"tight": np.diag([1e-8, 1e-10, 1e-12]), "medium": np.diag([1e-2, 4e-2, 1e-4]), "full": spd(rng, 3, 1e-3, 1e-1)}
    out = []
    for tag, cov in covs.items():
        sd = np.sqrt(np.diag(cov))
        params, pts = [], []
        for i, (th, wt) in enumerate(heading_plan(rng)):                       # the prior: the observation is prior pose
            reach = (1.0, 100.0, 1.0e4)[i % 3]
            xy = f32(rng.uniform(-reach, reach, 2))
            res = 2.0 * sd[:2] * rng.randn(2)
            pth = to_double(mpf(th) - mpf(wt))
            c, s = mp.cos(mpf(pth)), mp.sin(mpf(pth))
            px = to_double(mpf(xy[0]) - (c * mpf(res[0]) - s * mpf(res[1])))
            py = to_double(mpf(xy[1]) - (s * mpf(res[0]) + c * mpf(res[1])))
            params.append([px, py, pth] + list(cov.ravel()))
            pts.append([xy[0], xy[1], th])
        out.append(("se2_prior_" + tag, SE2[0], np.array(params), np.array(pts, dtype=np.float32)))
        params, pts = [], []
        for i, (thj, wt) in enumerate(heading_plan(rng)):
            reach = (1.0, 100.0, 1.0e4)[i % 3]
            thi = float(np.float32((0.0, rng.uniform(-np.pi, np.pi), REPRESENTATIVES[i % len(REPRESENTATIVES)])[(i // 2) % 3]))
            a = f32(rng.uniform(-reach, reach, 2))
            b = f32(a + rng.uniform(-5.0, 5.0, 2))
            res = 2.0 * sd[:2] * rng.randn(2)
            oth = to_double(mpf(thj) - mpf(thi) - mpf(wt))
            ci, si = mp.cos(mpf(thi)), mp.sin(mpf(thi))
            dx, dy = mpf(b[0]) - mpf(a[0]), mpf(b[1]) - mpf(a[1])
            ux, uy = ci * dx + si * dy, ci * dy - si * dx
            co, so = mp.cos(mpf(oth)), mp.sin(mpf(oth))
            ox = to_double(ux - (co * mpf(res[0]) - so * mpf(res[1])))
            oy = to_double(uy - (so * mpf(res[0]) + co * mpf(res[1])))
            params.append([ox, oy, oth] + list(cov.ravel()))
            pts.append([a[0], a[1], thi, b[0], b[1], thj])
        out.append(("se2_rel_" + tag, SE2[1], np.array(params), np.array(pts, dtype=np.float32)))
    # a loose prior (sigma of the heading 3 rad, precision 1/9) at a heading of 0 and offsets of centimetres: the score's
    # heading component is l'(w) and little else, so the bound there is the rounding of w against pi times l'' = 1/6.  w sweeps
    # the range in which a small-angle switch could sit: densely over [2e-3, 4e-3], then up to the switch at 0.2
    rng = np.random.RandomState(20261021)
    cov = np.diag([1.0, 1.0, 9.0])
    sweep = np.concatenate([np.geomspace(2.0e-3, 4.0e-3, 24), np.geomspace(4.0e-3, 0.199, 24)]) * np.where(np.arange(48) % 2, -1.0, 1.0)
    params, pts = [], []
    for wt in sweep:
        xy = f32(rng.uniform(-1.0, 1.0, 2))
        res = 0.05 * rng.randn(2)
        pth = -float(wt)
        c, s = mp.cos(mpf(pth)), mp.sin(mpf(pth))
        params.append([to_double(mpf(xy[0]) - (c * mpf(res[0]) - s * mpf(res[1]))),
                       to_double(mpf(xy[1]) - (s * mpf(res[0]) + c * mpf(res[1]))), pth] + list(cov.ravel()))
        pts.append([xy[0], xy[1], 0.0])
    out.append(("se2_prior_loose", SE2[0], np.array(params), np.array(pts, dtype=np.float32)))
    return out


DENORMAL = float(np.float32(1.4e-45))


def range_rows(rng, n, d, sigma, width_a):
    """[a | b] float32 with b on a ring around a, and the edge rows: separations of 0 (2 of n), a denormal, 1e19 per coordinate."""
    a = rng.uniform(-30, 30, (n, width_a))
    phi, r = rng.uniform(-np.pi, np.pi, n), np.abs(d + sigma * rng.randn(n) * np.where(np.arange(n) % 3 == 0, 5.0, 1.0))
    x = f32(np.concatenate([a, a[:, :2] + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)], 1))
    b = width_a
    x[0, b:b + 2] = x[0, :2]
    x[1, :2], x[1, b:b + 2] = (0.0, 0.0), (0.0, 0.0)
    x[2, :2], x[2, b:b + 2] = (0.0, 0.0), (DENORMAL, 0.0)                      # one float32 denormal apart
    x[3, :2], x[3, b:b + 2] = (0.0, 0.0), (-DENORMAL, DENORMAL)
    x[4, :2], x[4, b:b + 2] = (0.0, 0.0), (1e19, 1e19)                         # 1e19 per coordinate
    x[5, :2], x[5, b:b + 2] = (1e19, -1e19), (-1e19, 1e19)
    return f32(x)


def simple_cases(rng):
    out = []
    n = 48
    out.append(("range_pose_edges", "SE2R2RangeGaussianLikelihoodFactor", [[5.0, 0.5]], range_rows(rng, n, 5.0, 0.5, 3)))
    out.append(("range_pose_zero_measured", "SE2R2RangeGaussianLikelihoodFactor", [[0.0, 0.3]], range_rows(rng, n, 0.0, 0.3, 3)))
    out.append(("range_points_edges", "R2RangeGaussianLikelihoodFactor", [[12.0, 0.05]], range_rows(rng, n, 12.0, 0.05, 2)))
    for name, centre, mu, sigma in (("ring_edges", (0.0, 0.0), 5.0, 0.5), ("ring_zero_measured", (0.0, 0.0), 0.0, 2.0),
                                    ("ring_far_centre", (1.0e4, -4.0e3), 3.0, 0.1)):
        x = range_rows(rng, n, mu, sigma, 2)
        if centre != (0.0, 0.0):
            x = x[[0] + list(range(6, n))]                                      # (a denormal is lost next to 1e4)
        out.append((name, "UnaryR2RangeGaussianPriorFactor", [list(centre) + [mu, sigma]],
                    f32(x[:, 2:] - x[:, :2] + np.array(centre))))

    def mixture_rows(k_land, d, sigma, m=40):
        pose = np.stack([rng.uniform(-10, 10, m), rng.uniform(-10, 10, m), rng.uniform(-3 * np.pi, 3 * np.pi, m)], 1)
        lm = rng.uniform(-15, 15, (m, 2 * k_land))
        for i in range(m):
            j = i % k_land
            phi, r = rng.uniform(-np.pi, np.pi), d + sigma * rng.randn() * (1.0 + 4.0 * (i % 5 == 0))
            lm[i, 2 * j:2 * j + 2] = pose[i, :2] + r * np.array([np.cos(phi), np.sin(phi)])
        return f32(np.concatenate([pose, lm], 1))

    ada = "AmbiguousDataAssociationFactor"
    x = mixture_rows(1, 6.0, 0.5)
    x[0, 3:5] = x[0, :2]                                                        # the one candidate on the pose: masked
    out.append(("mix_k1", ada, [[1, 1.0, 6.0, 0.5, 0]], x))
    x = mixture_rows(2, 6.0, 0.5)
    x[:20, 5:7] = x[:20, 3:5]                                                   # tied: both candidates in one place
    x[20:30, 5:7] = x[20:30, :2] + (x[20:30, :2] - x[20:30, 3:5])               # tied: the same range, the opposite bearing
    out.append(("mix_k2_tied", ada, [[2, 0.5, 0.5, 6.0, 0.5, 0, 1]], f32(x)))
    x = mixture_rows(3, 11.0, 1.0)
    for i in range(0, 40, 2):                                                   # one component ahead by 1e4 in the log:
        j = i % 3                                                               # the others sqrt(2e4) sigma off their range
        for o in range(3):
            if o != j:
                phi = rng.uniform(-np.pi, np.pi)
                x[i, 3 + 2 * o:5 + 2 * o] = x[i, :2] + (11.0 + np.sqrt(2.0e4)) * np.array([np.cos(phi), np.sin(phi)])
    out.append(("mix_k3_ahead", ada, [[3, 0.2, 0.5, 0.3, 11.0, 1.0, 0, 1, 2]], f32(x)))
    x = mixture_rows(4, 4.0, 0.4)
    for i in range(20):                                                         # every candidate 1e4 m away, each further
        for o in range(4):                                                      # than the last by 10 % (no tie out there)
            phi = rng.uniform(-np.pi, np.pi)
            x[i, 3 + 2 * o:5 + 2 * o] = x[i, :2] + 1.0e4 * (1.0 + 0.1 * ((o + i) % 4)) * np.array([np.cos(phi), np.sin(phi)])
    out.append(("mix_k4_far", ada, [[4, 0.1, 0.2, 0.3, 0.4, 4.0, 0.4, 0, 1, 2, 3]], f32(x)))
    out.append(("mix_twice", ada, [[3, 0.5, 0.3, 0.2, 7.0, 0.6, 0, 1, 0]], mixture_rows(2, 7.0, 0.6)))
    out.append(("mix_tiny_weight", ada, [[2, 1.0, 1e-300, 6.0, 0.5, 0, 1]], mixture_rows(2, 6.0, 0.5)))
    x = range_rows(rng, 40, 8.0, 0.5 * np.sqrt(10.0), 3)[[0] + list(range(6, 40))]
    out.append(("null_hypo", "BinaryFactorWithNullHypo", [[0.9, 0.1, 8.0, 0.5, 10.0]], x))

    rho = 0.999999
    cov = np.array([[4e-2, rho * 2e-1 * 3e-1], [rho * 2e-1 * 3e-1, 9e-2]])
    chol = np.linalg.cholesky(cov)
    mu = np.array([12.5, -7.0])
    out.append(("r2_prior_corr", "UnaryR2GaussianPriorFactor", [list(mu) + list(cov.ravel())],
                f32(mu + rng.randn(40, 2) @ chol.T * 0.5)))                # (half a sigma: the bound grows with the square)
    cov2 = spd(rng, 2, 1e-2, 4.0)
    far = rng.randn(40, 2)
    far = 1.0e4 * far / np.sqrt((far ** 2).sum(1))[:, None] * np.sqrt(np.diag(cov2))
    out.append(("r2_prior_far", "UnaryR2GaussianPriorFactor", [list(mu) + list(cov2.ravel())], f32(mu + far)))
    obs = np.array([-3.5, 0.25])
    a = rng.uniform(-1.0e4, 1.0e4, (40, 2))
    out.append(("r2_rel_corr", "R2RelativeGaussianLikelihoodFactor", [list(obs) + list(cov.ravel())],
                f32(np.concatenate([a, a + obs + rng.randn(40, 2) @ chol.T * 0.5], 1))))
    a = rng.uniform(-20, 20, (40, 2))
    out.append(("r2_rel_far", "R2RelativeGaussianLikelihoodFactor", [list(obs) + list(cov2.ravel())],
                f32(np.concatenate([a, a + obs + far], 1))))
    return [(name, cls, np.array(p, dtype=np.float64), np.asarray(x, dtype=np.float32)) for name, cls, p, x in out]


def all_cases():
    """[(name, class, params [m or 1, p], x float32 [m, width])]: part (a) of factor_density.npz, then the new cases."""
    dens = np.load(DENSITY)
    out = [("a%03d" % i, str(cls), dens["a%03d_params" % i][None, :], dens["a%03d_x" % i])
           for i, cls in enumerate(dens["a_classes"])]
    rng = np.random.RandomState(20261020)
    return out + se2_cases(rng) + simple_cases(rng)


# ---- whole graphs -----------------------------------------------------------------------------------------------------------------
def parse_factor(line):
    """A `Factor ...` line of a .fg file -> (class, variable names in the factor's column order, constructor parameters)."""
    t = line.split()[1:]
    if t[0] == SE2[0]:
        assert t[5] == "covariance"
        return t[0], [t[1]], [float(v) for v in t[2:5] + t[6:15]]
    if t[0] == SE2[1]:
        assert t[6] == "covariance"
        return t[0], t[1:3], [float(v) for v in t[3:6] + t[7:16]]
    if t[0] == "SE2R2RangeGaussianLikelihoodFactor":
        return t[0], t[1:3], [float(t[3]), float(t[4])]
    if t[0] == "AmbiguousDataAssociationFactor":
        i_seen, i_w, i_cls, i_obs, i_sig = (t.index(k) + 1 for k in ("Observed", "Weights", "Binary", "Observation", "Sigma"))
        seen = t[i_seen:i_w - 1]
        uniq = [v for i, v in enumerate(seen) if v not in seen[:i]]
        ws = [float(v) for v in t[i_w:i_cls - 1]]
        assert t[i_cls] == "SE2R2RangeGaussianLikelihoodFactor"
        return t[0], [t[t.index("Observer") + 1]] + uniq, [len(seen)] + ws + [float(t[i_obs]), float(t[i_sig])] + \
            [uniq.index(v) for v in seen]
    raise KeyError(t[0])


def graph_values(factors, col, width, x, what):
    """factors [(class, variable names, parameters)], col {name: (column, dim)} -> per-factor terms, the total and the joint
    score with scales and allowances at the rows of x."""
    n = x.shape[0]
    terms = [[None] * n for _ in factors]
    tot = [[R(0), mpf(0)] for _ in range(n)]
    score = [[R(0)] * width for _ in range(n)]
    for fi, (cls, names, p) in enumerate(factors):
        cols = [c for v in names for c in range(col[v][0], col[v][0] + col[v][1])]
        for r in range(n):
            got = evaluate(cls, p, x[r, cols])
            assert got["mask"], (what, fi, r)                     # no graph point sits at a range of exactly 0
            assert got["w"] is None or mp.pi - abs(got["w"]) > mpf("1e-6"), (what, fi, r)
            if (fi + r) % 7 == 0:
                cross_check(cls, p, x[r, cols], got, (what, fi, r))
            terms[fi][r] = got
            tot[r][0] = tot[r][0] + R(got["logp"], got["logp_scale"])
            tot[r][1] += got["logp_allow"]
            for c, g, e in zip(cols, got["score"], got["score_scale"]):
                score[r][c] = score[r][c] + R(g, e)
        if fi % 200 == 0:
            print("  %s: factor %d of %d" % (what, fi, len(factors)), flush=True)
    return terms, tot, score


def up32(a):
    """float32, rounded up: a stored scale is never below the 60-digit one."""
    a = np.asarray(a, dtype=np.float64)
    f = a.astype(np.float32)
    low = f.astype(np.float64) < a
    f[low] = np.nextafter(f[low], np.float32(np.inf))
    return f


def up64(values):
    """float64, rounded up (the cases' scales: 1e19 m squared is past float32)."""
    return np.array([float(v) * (1.0 + 2.0 ** -52) for v in values], dtype=np.float64)


def to_f64(rows):
    return np.array([[float(v) for v in row] for row in rows], dtype=np.float64)


def check_caps(name, exact, scale, what):
    exact, scale = np.asarray(exact, dtype=np.float64).ravel(), np.asarray(scale, dtype=np.float64).ravel()
    bound = C_BOUND * EPS * scale
    assert np.all(np.isfinite(exact)) and np.all(np.isfinite(scale)), (name, what)
    assert np.all(bound <= VACUOUS * (np.abs(exact) + 1.0)), (name, what, float(np.max(bound / (np.abs(exact) + 1.0))))
    share = float(np.mean(bound <= CAP * (np.abs(exact) + 1.0))) if exact.size else 1.0
    if name not in EXEMPT:
        assert share >= 0.9, (name, what, share)
    return share


def main():
    out, names = {}, []
    for name, cls, params, x in all_cases():
        assert x.shape[0] <= 64 and params.shape[0] in (1, x.shape[0]), name
        rows = [evaluate(cls, params[i % params.shape[0]], x[i]) for i in range(x.shape[0])]
        for i, got in enumerate(rows):
            cross_check(cls, params[i % params.shape[0]], x[i], got, (name, i))
            assert got["w"] is None or mp.pi - abs(got["w"]) > mpf("1e-6"), (name, i, "a point on the heading wrap")
        mask = np.array([r["mask"] for r in rows])
        assert (~mask).sum() <= 0.05 * mask.size, (name, int((~mask).sum()), mask.size)
        names.append(name)
        if not name.startswith("a0"):
            out[name + "_cls"], out[name + "_params"], out[name + "_x"] = np.array(cls), params, x
        out[name + "_logp"] = np.array([float(r["logp"]) for r in rows])
        out[name + "_logp_scale"] = up64([r["logp_scale"] for r in rows])
        out[name + "_logp_allow"] = np.array([float(r["logp_allow"]) for r in rows])
        out[name + "_score"] = to_f64([r["score"] for r in rows])
        out[name + "_score_scale"] = np.stack([up64(r["score_scale"]) for r in rows])
        out[name + "_mask"] = mask
        if cls in SE2:
            out[name + "_w"] = np.array([float(r["w"]) for r in rows])
        s_v = check_caps(name, out[name + "_logp"], out[name + "_logp_scale"], "value")
        s_g = check_caps(name, out[name + "_score"][mask], out[name + "_score_scale"][mask], "score")
        print("%-26s %-42s rows %2d masked %d   within the 1e-9 cap: value %.2f score %.2f%s"
              % (name, cls, x.shape[0], int((~mask).sum()), s_v, s_g, "   (exempt)" if name in EXEMPT else ""), flush=True)
    out["cases"] = np.array(names)
    out["exempt"] = np.array(sorted(EXEMPT))
    out["exempt_reason"] = np.array([EXEMPT[k] for k in sorted(EXEMPT)])

    dens, sc = np.load(DENSITY), np.load(SCORE)
    graphs = []
    for key, (folder, pick) in GRAPHS.items():
        col, off = {}, 0
        for v, d in zip(dens[key + "_vars"], dens[key + "_dims"]):
            col[str(v)] = (off, int(d))
            off += int(d)
        with open(os.path.join(DATA, folder, "factor_graph.fg")) as f:
            factors = [parse_factor(ln) for ln in f if ln.startswith("Factor ")]
        assert [cls + " " + " ".join(nm) for cls, nm, p in factors] == [str(s) for s in dens[key + "_factors"]]
        rows = sc[key + "_rows"][pick]
        graphs.append((key, factors, col, off, rows, dens[key + "_x"][rows]))
    truth = sc["ksd_truth"]

    def dist(a, b):
        return float(np.sqrt(((truth[a:a + 2] - truth[b:b + 2]) ** 2).sum()))
    odo = list(np.diag([0.04, 0.04, 0.01]).ravel())
    ksd = [(SE2[0], ["X0"], [0.0, 0.0, 0.0] + list(np.diag([0.01, 0.01, 0.0025]).ravel())),
           (SE2[1], ["X0", "X1"], [2.0, 0.0, 0.5] + odo), (SE2[1], ["X1", "X2"], [1.8, 0.16, 0.7] + odo)]
    ksd += [("SE2R2RangeGaussianLikelihoodFactor", ["X%d" % a, "L%d" % b], [dist(3 * a, 9 + 2 * b), 0.3])
            for a, b in ((0, 0), (1, 0), (1, 1), (2, 1))]
    ksd.append(("AmbiguousDataAssociationFactor", ["X2", "L0", "L1"], [2, 0.5, 0.5, dist(6, 9), 0.3, 0, 1]))
    assert [cls + " " + " ".join(nm) for cls, nm, p in ksd] == [str(s) for s in sc["ksd_factors"]]
    graphs.append(("ksd", ksd, {"X0": (0, 3), "X1": (3, 3), "X2": (6, 3), "L0": (9, 2), "L1": (11, 2)}, 13,
                   np.arange(KSD_POINTS), sc["ksd_samples"][:KSD_POINTS]))
    for key, factors, col, width, rows, x in graphs:
        terms, tot, score = graph_values(factors, col, width, x, key)
        out[key + "_rows"] = np.asarray(rows, dtype=np.int32)
        out[key + "_terms"] = to_f64([[g["logp"] for g in row] for row in terms])
        out[key + "_terms_scale"] = up32(to_f64([[g["logp_scale"] for g in row] for row in terms]))
        out[key + "_terms_allow"] = to_f64([[g["logp_allow"] for g in row] for row in terms])
        out[key + "_total"] = np.array([float(t[0].v) for t in tot])
        out[key + "_total_scale"] = up32([float(t[0].e) for t in tot])
        out[key + "_total_allow"] = np.array([float(t[1]) for t in tot])
        out[key + "_score"] = to_f64([[g.v for g in row] for row in score])
        out[key + "_score_scale"] = up32(to_f64([[g.e for g in row] for row in score]))
        shares = [check_caps(key, out[key + a], out[key + a + "_scale"], a) for a in ("_terms", "_total", "_score")]
        print("%-14s %4d factors x %2d points   within the 1e-9 cap: terms %.3f totals %.2f score %.3f"
              % (key, len(factors), x.shape[0], *shares), flush=True)
    out["graphs"] = np.array([g[0] for g in graphs])
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes;", len(names), "cases")
    assert size < os.path.getsize(SCORE), "the fixture must stay below factor_score.npz"


if __name__ == "__main__":
    sys.exit(main())
