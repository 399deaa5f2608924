#!/usr/bin/env python3
"""The Hessians of the factor densities to 60 digits: the third row of value / score / curvature, for the cases and the points
of tests/golden/factor_exact.npz (neither is stored again).  python + mpmath, no GPU; like make_factor_exact_fixture.py, which
this script imports for `plain_log_pdf`, the running-bound arithmetic `R`, `all_cases()`, the graph readers and the constants
of `check_caps` (C_BOUND, CAP, EPS; the cap itself is restated in `base_check`: the EXEMPT table here has one more row), it reads nothing of factors/Factors.py or csrc/factor_model.h.

Writes tests/golden/factor_hessian_exact.npz, the yardstick of `Factors.*.hess_x_log_pdf` and of the device entry
`nfisam_factor_graph_hvp` (tests/test_factor_hessian_cpu.py, tests/test_factor_hessian_gpu.py).

What is evaluated: the second derivatives of the SMOOTH densities of that generator's docstring, at the float32 points.  Two
evaluations of every block [w, w] are made and must agree to 1e-20 of (scale + 1) at every case point:
  * the second-order `mpmath.diff` of `plain_log_pdf` (upper triangle; the block is symmetric);
  * column c of the block as the derivative of the analytic GRADIENT along e_c: the gradient formulas of `se2_tangent`,
    `range_term` and `eval_mixture` once more, on pairs (value, derivative along the direction) whose two halves are `R`
    values -- class J.  Every rule of `R` then holds for the derivative half as it stands: a product rule's two summands add
    their bounds, a quotient's likewise, a function f(u) contributes f'(u) du with f' bounded through f''.  The log-map terms
    a, a', l' count as functions of w, so their derivatives along the direction are a' dw, a'' dw, l'' dw with
        a''  = (a - 1) / (2 sin^2 h),              l''  = (1 / sin^2 h - 1 / h^2) / 2                 (h = w / 2)
        a''' = (a' - (a - 1) cot h) / (2 sin^2 h),  l''' = (1 / h^3 - cot h / sin^2 h) / 2
    (limits at w = 0: -1/6, 1/6, 0, 0), the third derivatives bounding the second ones as functions of w.  These six are
    evaluated at 140 digits: l''' cancels 48 of them at |w| = 1e-12.
    The heading residual w has derivative exactly 1 in th (prior), -1 / +1 in th_i / th_j (relative pose).
What is stored, per case, as float64 rounded from 60 digits:
    <name>_hess        [m, w, w] in the factor's own column order; a masked row (a range of exactly 0, the mask of
                       factor_exact.npz) stores 0: the score is the zero vector there, and so is its derivative;
    <name>_hess_scale  the running bound, rounded up and made symmetric (the larger of [r, c] and [c, r]: the two columns
                       reach the entry along different chains).
Whole graphs -- `ksd` (13 columns, the 64 stored points) and `manhattan136` at every sixth of the rows factor_exact.npz names:
    <key>_v         one fixed direction per graph [total_dim] float64 (seeded, standard normal);
    <key>_hv        the exact joint product sum_c H[r, c] v[c], [n, total_dim]: every factor's block times v on its columns,
                    added per row in table order;
    <key>_hv_scale  its running bound (float32, rounded up): the product enters with the sum of the magnitudes of its
                    summands (the rules of `R`, the direction being v instead of e_c).

Caps asserted of the output (fixed before anything was measured): masked rows unchanged (<= 5 %, only at a range of exactly
0); 256 x 2^-53 x scale <= 1e-9 (|exact| + 1) on at least 90 % of the entries of every case that EXEMPT does not name; the
file is no larger than factor_exact.npz.

    python tests/golden/make_factor_hessian_fixture.py [processes]
"""
import importlib.util
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_factor_exact_fixture", os.path.join(HERE, "make_factor_exact_fixture.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)                      # (sets mp.dps = 60)
R, SE2 = base.R, base.SE2

OUT = os.path.join(HERE, "factor_hessian_exact.npz")
EXACT = os.path.join(HERE, "factor_exact.npz")
AGREE = mpf("1e-20")
GRAPH_PICK = {"ksd": slice(0, None), "manhattan136": slice(0, None, 6)}
V_SEED = 20261022
# the cases that miss the 1e-9 cap, and why: those of the value's and the score's table, for their reasons squared
EXEMPT = {
    "a000": "prior with covariance diag(1e-8, 1e-10, 1e-12): entries of 1e12 carry the heading's rounding against pi",
    "a001": "prior with covariance diag(1e-4, 1e-6, 1e-8), heading next to +pi: the same, precision 1e8",
    "a004": "relative pose with the isotropic covariance 1e-4 I: the x-y entries are c s P - s c P, two products of 1e4 that "
            "cancel to (nearly) 0: the bound 256 x 2^-53 x 1e4 = 2.7e-9 is absolute there, against |exact| + 1 = 1",
    "se2_prior_tight": "covariance diag(1e-8, 1e-10, 1e-12)",
    "se2_rel_tight": "covariance diag(1e-8, 1e-10, 1e-12), offsets of metres against residuals of 1e-4 m",
    "r2_prior_corr": "correlation 0.999999: the determinant 1 - rho^2 cancels six digits of every entry of the precision",
    "r2_rel_corr": "correlation 0.999999: the same constant blocks",
}


# ---- (value, derivative along one direction), both halves with their running bounds --------------------------------------------
class J(object):
    __slots__ = ("v", "d")

    def __init__(self, v, d=0):
        self.v, self.d = R.of(v), R.of(d)

    @staticmethod
    def of(a):
        return a if isinstance(a, J) else J(a)

    def __add__(self, o):
        o = J.of(o)
        return J(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = J.of(o)
        return J(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return J.of(o) - self

    def __neg__(self):
        return J(-self.v, -self.d)

    def __mul__(self, o):
        o = J.of(o)
        return J(self.v * o.v, self.d * o.v + self.v * o.d)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = J.of(o)
        q = self.v / o.v
        return J(q, self.d / o.v - q * o.d / o.v)

    def fun(self, f, df, ddf):
        """f(self): value f, first derivative df, second ddf (the bound of df as a function of self.v)."""
        return J(self.v.fun(f, df), self.v.fun(df, ddf) * self.d)


def j_sin(a):
    s, c = mp.sin(a.v.v), mp.cos(a.v.v)
    return a.fun(s, c, s)


def j_cos(a):
    s, c = mp.sin(a.v.v), mp.cos(a.v.v)
    return a.fun(c, -s, c)


def j_log(a):
    return a.fun(mp.log(a.v.v), 1 / a.v.v, 1 / a.v.v ** 2)


def j_exp(a):
    e = mp.exp(a.v.v)
    return a.fun(e, e, e)


def j_sqrt(a):
    s = mp.sqrt(a.v.v)
    return a.fun(s, 1 / (2 * s), 1 / (4 * s ** 3))


def j_total(items):
    acc = J(0)
    for it in items:
        acc = acc + it
    return acc


def j_gaussian_parts(cov):
    prec, log_norm = base.gaussian_parts(cov)                       # constants: no derivative half
    return [[J(p) for p in row] for row in prec]


def log_map_derivatives(x):
    """a, a', a'', a''', l', l'', l''' at the heading residual x (mpf), computed at 140 digits."""
    with mp.workdps(140):
        if x == 0:
            out = (mpf(1), mpf(0), -mpf(1) / 6, mpf(0), mpf(0), mpf(1) / 6, mpf(0))
        else:
            h = x / 2
            cot, s2 = mp.cot(h), 1 / mp.sin(h) ** 2
            a = h * cot
            da = (cot - h * s2) / 2
            out = (a, da, (a - 1) * s2 / 2, (da - (a - 1) * cot) * s2 / 2, 1 / h - cot, (s2 - 1 / h ** 2) / 2,
                   (1 / h ** 3 - cot * s2) / 2)
        out = tuple(+t for t in out)
    return tuple(+t for t in out)                                    # rounded to the 60 digits of the rest


def j_log_map_terms(w):
    """a(w), a'(w), l'(w) as J values of the J value w."""
    a, da, dda, ddda, dl, ddl, dddl = log_map_derivatives(w.v.v)
    return w.fun(a, da, dda), w.fun(da, dda, ddda), w.fun(dl, ddl, dddl)


def j_se2_tangent_grad(tx, ty, w, cov):
    """The gradient of `se2_tangent` of make_factor_exact_fixture.py, on J values."""
    prec = j_gaussian_parts(cov)
    a, da, dl = j_log_map_terms(w)
    h = w * 0.5
    v = [a * tx + h * ty, a * ty - h * tx, w]
    pv = [j_total(prec[i][j] * v[j] for j in range(3)) for i in range(3)]
    gtx = -(a * pv[0] - h * pv[1])
    gty = -(h * pv[0] + a * pv[1])
    gw = dl - (pv[0] * (da * tx + ty * 0.5) + pv[1] * (da * ty - tx * 0.5) + pv[2])
    return gtx, gty, gw


def j_in(x, v):
    """the float32 point x (mpf) with the direction v (R values or numbers) -> J inputs: exact values, as given directions."""
    return [J(R(xi), vi) for xi, vi in zip(x, v)]


def grad_se2_prior(p, x, v):
    px, py, pth = (R(float(t)) for t in p[:3])
    cov = np.asarray(p[3:12], dtype=np.float64).reshape(3, 3)
    c, s = J(base.r_cos(pth)), J(base.r_sin(pth))
    X = j_in(x, v)
    dx, dy = X[0] - px, X[1] - py
    tx, ty = c * dx + s * dy, c * dy - s * dx
    wv = base.reduce_heading(x[2] - pth.v)
    w = J(R(wv, abs(x[2]) + abs(pth.v) + mp.pi), X[2].d)            # d w / d th = 1
    gtx, gty, gw = j_se2_tangent_grad(tx, ty, w, cov)
    return [c * gtx - s * gty, s * gtx + c * gty, gw], True


def grad_se2_relative(p, x, v):
    ox, oy, oth = (R(float(t)) for t in p[:3])
    cov = np.asarray(p[3:12], dtype=np.float64).reshape(3, 3)
    X = j_in(x, v)
    thi, thj = X[2], X[5]
    ci, si, co, so = j_cos(thi), j_sin(thi), J(base.r_cos(oth)), J(base.r_sin(oth))
    dx, dy = X[3] - X[0], X[4] - X[1]
    ux, uy = ci * dx + si * dy, ci * dy - si * dx
    rx, ry = ux - ox, uy - oy
    tx, ty = co * rx + so * ry, co * ry - so * rx
    wv = base.reduce_heading(x[5] - x[2] - oth.v)
    w = J(R(wv, abs(x[2]) + abs(x[5]) + abs(oth.v) + mp.pi), thj.d - thi.d)
    gtx, gty, gw = j_se2_tangent_grad(tx, ty, w, cov)
    grx, gry = co * gtx - so * gty, so * gtx + co * gty
    gbx, gby = ci * grx - si * gry, si * grx + ci * gry
    return [-gbx, -gby, grx * uy - gry * ux - gw, gbx, gby, gw], True


def j_range_term(ax, ay, bx, by, d, sigma):
    """(log N(|a - b| - d; 0, sigma^2), its gradient in a) on J values; the gradient is None at |a - b| = 0."""
    dx, dy = ax - bx, ay - by
    var = J(R(float(sigma)) * R(float(sigma)))
    if dx.v.v == 0 and dy.v.v == 0:
        return J(-(base.r_log(R(2 * mp.pi) * var.v)) * 0.5 - R(float(d)) * R(float(d)) / var.v * 0.5), None
    r = j_sqrt(dx * dx + dy * dy)
    delta = r - R(float(d))
    value = J(-(base.r_log(R(2 * mp.pi) * var.v)) * 0.5) - delta * delta / var * 0.5
    coef = -(delta / var) / r
    return value, (coef * dx, coef * dy)


def grad_range(p, x, v, pose):
    o = 3 if pose else 2
    X = j_in(x, v)
    _, g = j_range_term(X[0], X[1], X[o], X[o + 1], p[0], p[1])
    if g is None:
        return [J(0)] * (o + 2), False
    return [g[0], g[1]] + ([J(0)] if pose else []) + [-g[0], -g[1]], True


def grad_ring(p, x, v):
    X = j_in(x, v)
    _, g = j_range_term(X[0], X[1], J(R(float(p[0]))), J(R(float(p[1]))), p[2], p[3])
    if g is None:
        return [J(0), J(0)], False
    return [g[0], g[1]], True


def grad_mixture(weights, cands, ds, sigmas, x, v, n_landmarks):
    X = j_in(x, v)
    wsum = base.total(R(float(t)) for t in weights)
    terms, grads, ok = [], [], True
    for wj, cj, dj, sj in zip(weights, cands, ds, sigmas):
        value, g = j_range_term(X[0], X[1], X[3 + 2 * cj], X[4 + 2 * cj], dj, sj)
        ok = ok and g is not None
        terms.append(value + J(base.r_log(R(float(wj)) / wsum)))
        grads.append(g)
    out = [J(0)] * (3 + 2 * n_landmarks)
    if not ok:
        return out, False
    top = max(range(len(terms)), key=lambda j: terms[j].v.v)
    es = [j_exp(terms[j] - terms[top]) for j in range(len(terms))]   # (the top one: exp(0) = 1, its derivative half 0)
    acc = j_total(es)
    for j, cj in enumerate(cands):
        rj = es[j] / acc
        gx, gy = rj * grads[j][0], rj * grads[j][1]
        out[0], out[1] = out[0] + gx, out[1] + gy
        out[3 + 2 * cj], out[4 + 2 * cj] = out[3 + 2 * cj] - gx, out[4 + 2 * cj] - gy
    return out, True


def grad_r2(mu, cov, d):
    prec, _ = base.gaussian_parts(cov)
    res = [d[0] - R(float(mu[0])), d[1] - R(float(mu[1]))]
    return [-j_total(J(prec[i][j]) * res[j] for j in range(2)) for i in range(2)]


def gradient_along(cls, p, x, v):
    """The analytic gradient of one factor at the float32 point x (mpf) and its derivative along v -> ([J], mask)."""
    if cls == SE2[0]:
        return grad_se2_prior(p, x, v)
    if cls == SE2[1]:
        return grad_se2_relative(p, x, v)
    if cls == "SE2R2RangeGaussianLikelihoodFactor":
        return grad_range(p, x, v, True)
    if cls == "R2RangeGaussianLikelihoodFactor":
        return grad_range(p, x, v, False)
    if cls == "UnaryR2RangeGaussianPriorFactor":
        return grad_ring(p, x, v)
    if cls == "AmbiguousDataAssociationFactor":
        k = int(p[0])
        cands = [int(t) for t in p[3 + k:3 + 2 * k]] if len(p) > 3 + k else list(range(k))
        return grad_mixture(p[1:1 + k], cands, [p[1 + k]] * k, [p[2 + k]] * k, x, v, max(cands) + 1)
    if cls == "BinaryFactorWithNullHypo":
        return grad_mixture(p[:2], [0, 0], [p[2]] * 2, [p[3], p[3] * p[4]], x, v, 1)
    if cls == "UnaryR2GaussianPriorFactor":
        X = j_in(x, v)
        return grad_r2(p[:2], np.array(p[2:6]).reshape(2, 2), [X[0], X[1]]), True
    if cls == "R2RelativeGaussianLikelihoodFactor":
        X = j_in(x, v)
        g = grad_r2(p[:2], np.array(p[2:6]).reshape(2, 2), [X[2] - X[0], X[3] - X[1]])
        return [-g[0], -g[1], g[0], g[1]], True
    raise KeyError(cls)


def hessian(cls, p, x):
    """One factor at the float32 point x -> dict: hess, hess_scale ([w][w] of mpf, scale symmetric), mask."""
    p = [float(t) for t in p]
    x = [mpf(float(t)) for t in x]
    n = len(x)
    cols = []
    for c in range(n):
        g, ok = gradient_along(cls, p, x, [1 if j == c else 0 for j in range(n)])
        cols.append(g)
    if not ok:
        zero = [[mpf(0)] * n for _ in range(n)]
        return dict(hess=zero, hess_scale=zero, mask=False)
    hess = [[cols[c][r].d.v for c in range(n)] for r in range(n)]
    scale = [[max(cols[c][r].d.e, cols[r][c].d.e) for c in range(n)] for r in range(n)]
    return dict(hess=hess, hess_scale=scale, mask=True, asym=max(abs(hess[r][c] - hess[c][r]) / (scale[r][c] + 1)
                                                                 for r in range(n) for c in range(n)))


def product(cls, p, x, v):
    """H v of one factor along the float64 direction v -> [R]: value and running bound per column of the factor."""
    p = [float(t) for t in p]
    g, ok = gradient_along(cls, p, [mpf(float(t)) for t in x], [R(float(t)) for t in v])
    assert ok
    return [t.d for t in g]


def cross_check(cls, p, x, got, what):
    """`hessian` against the second-order `mpmath.diff` of the plain definition: 1e-20 of (scale + 1), the upper triangle (the
    analytic block's own asymmetry is held to the same)."""
    if not got["mask"]:
        return
    assert got["asym"] <= AGREE, (what, "asymmetric", got["asym"])
    xs = tuple(mpf(float(t)) for t in x)
    n = len(xs)
    for r in range(n):
        for c in range(r, n):
            order = tuple((1 if j == r else 0) + (1 if j == c else 0) for j in range(n))
            if got["hess"][r][c] == 0 and got["hess_scale"][r][c] == 0 and cls not in SE2:
                continue                                              # a column the factor does not read (a pose's heading)
            d = mp.diff(lambda *a: base.plain_log_pdf(cls, p, a), xs, order)
            assert abs(d - got["hess"][r][c]) <= AGREE * (got["hess_scale"][r][c] + 1), (what, r, c, d, got["hess"][r][c])


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def do_case(job):
    name, cls, params, x = job
    rows = [hessian(cls, params[i % params.shape[0]], x[i]) for i in range(x.shape[0])]
    for i, got in enumerate(rows):
        cross_check(cls, params[i % params.shape[0]], x[i], got, (name, i))
    hess = np.array([[[float(t) for t in row] for row in r["hess"]] for r in rows])
    scale = np.array([[base.up64(row) for row in r["hess_scale"]] for r in rows])
    scale[~np.array([r["mask"] for r in rows])] = 0.0
    return name, hess, scale, np.array([r["mask"] for r in rows])


def do_graph_rows(job):
    key, factors, col, width, x = job
    out_v, out_e = [], []
    v = direction(key, width)
    for r in range(x.shape[0]):
        acc = [R(0)] * width
        for cls, names, p in factors:
            cols = [c for nm in names for c in range(col[nm][0], col[nm][0] + col[nm][1])]
            for c, t in zip(cols, product(cls, p, x[r, cols], v[cols])):
                acc[c] = acc[c] + t
        out_v.append([float(t.v) for t in acc])
        out_e.append([float(t.e) for t in acc])
    return key, np.array(out_v), np.array(out_e)


def direction(key, width):
    return np.random.RandomState(V_SEED + width).randn(width)


def graphs():
    """[(key, factors, col, width, x float32)]: the `ksd` graph and manhattan136 as make_factor_exact_fixture.py builds them."""
    dens, sc, fx = np.load(base.DENSITY), np.load(base.SCORE), np.load(EXACT)
    out = []
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
    rows = fx["ksd_rows"][GRAPH_PICK["ksd"]]
    out.append(("ksd", ksd, {"X0": (0, 3), "X1": (3, 3), "X2": (6, 3), "L0": (9, 2), "L1": (11, 2)}, 13, rows, sc["ksd_samples"][rows]))
    key, folder = "manhattan136", base.GRAPHS["manhattan136"][0]
    col, off = {}, 0
    for v, d in zip(dens[key + "_vars"], dens[key + "_dims"]):
        col[str(v)] = (off, int(d))
        off += int(d)
    with open(os.path.join(base.DATA, folder, "factor_graph.fg")) as f:
        factors = [base.parse_factor(ln) for ln in f if ln.startswith("Factor ")]
    assert [cls + " " + " ".join(nm) for cls, nm, p in factors] == [str(s) for s in dens[key + "_factors"]]
    rows = fx[key + "_rows"][GRAPH_PICK[key]]
    out.append((key, factors, col, off, rows, dens[key + "_x"][rows]))
    return out


def main():
    import multiprocessing
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else max(1, min(8, multiprocessing.cpu_count()))
    fx = np.load(EXACT)
    cases = base.all_cases()
    assert [c[0] for c in cases] == [str(n) for n in fx["cases"]]
    gs = graphs()
    jobs = [(key, factors, col, width, x[i:i + 1]) for key, factors, col, width, rows, x in gs for i in range(x.shape[0])]
    out = {}
    with multiprocessing.Pool(procs) as pool:
        graph_parts = pool.map_async(do_graph_rows, jobs, chunksize=1)
        for name, hess, scale, mask in pool.imap(do_case, sorted(cases, key=lambda c: -c[3].size)):
            assert np.array_equal(mask, fx[name + "_mask"]), name      # the masked rows: those of factor_exact.npz
            assert np.all(hess[~mask] == 0.0)
            out[name + "_hess"], out[name + "_hess_scale"] = hess, scale
            share = base_check(name, hess[mask], scale[mask])
            print("%-26s rows %2d masked %d   within the 1e-9 cap: %.2f%s"
                  % (name, mask.size, int((~mask).sum()), share, "   (exempt)" if name in EXEMPT else ""), flush=True)
        parts = graph_parts.get()
    out = {k: out[k] for name in fx["cases"] for k in (str(name) + "_hess", str(name) + "_hess_scale")}
    out["exempt"] = np.array(sorted(EXEMPT))
    out["exempt_reason"] = np.array([EXEMPT[k] for k in sorted(EXEMPT)])
    for key, factors, col, width, rows, x in gs:
        mine = [p for p in parts if p[0] == key]
        assert len(mine) == x.shape[0]
        out[key + "_rows"] = np.asarray(rows, dtype=np.int32)
        out[key + "_v"] = direction(key, width)
        out[key + "_hv"] = np.concatenate([p[1] for p in mine])
        out[key + "_hv_scale"] = base.up32(np.concatenate([p[2] for p in mine]))
        share = base_check(key, out[key + "_hv"], out[key + "_hv_scale"], graph=True)
        print("%-14s %4d factors x %2d points   within the 1e-9 cap: H v %.3f" % (key, len(factors), x.shape[0], share), flush=True)
    out["graphs"] = np.array([g[0] for g in gs])
    assert not MISSED, MISSED                                        # (every case is measured before the cap is asserted)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size <= os.path.getsize(EXACT), "the fixture must be no larger than factor_exact.npz"


MISSED = []


def base_check(name, exact, scale, graph=False):
    """The 1e-9 cap on 90 % of the entries (a case that EXEMPT names is only measured); every entry finite."""
    exact, scale = np.asarray(exact, dtype=np.float64).ravel(), np.asarray(scale, dtype=np.float64).ravel()
    assert np.all(np.isfinite(exact)) and np.all(np.isfinite(scale)) and np.all(scale >= 0), name
    share = float(np.mean(base.C_BOUND * base.EPS * scale <= base.CAP * (np.abs(exact) + 1.0))) if exact.size else 1.0
    if share < 0.9 and name not in EXEMPT:
        MISSED.append((name, share))
    return share


if __name__ == "__main__":
    sys.exit(main())
