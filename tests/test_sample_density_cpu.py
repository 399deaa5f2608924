"""Marginal densities at query points (nfisam_sample_density, utils.Statistics.sample_density, posterior_marginal_density) --
what needs no GPU: the float64 numpy oracle of the entry's formula against the same formula in mpmath at 50 digits and against
scipy's stored gaussian_kde.logpdf (tests/golden/sample_density.npz; this file imports no scipy), the bandwidth rules against
scipy's stored covariance, hpd_level, the leave-one-out selection, and every refusal.  The GPU tests
(test_sample_density_gpu.py) import the oracle from here.

THE FORMULA (include/nfisam_hip.h).  For query i and sample j of a block with whitening matrix W (lower triangular),
    diff_c = (double)x_jc - (double)q_ic (wrapped into [-pi, pi) on a circular entry),   u_r = sum_{c <= r} W_rc diff_c,
    e_ij = -1/2 sum_r u_r^2 + log_w[j],      log_dens_i = ((log_norm + M_i) + log S_i) - log W_tot,
    M_i = max_j e_ij,  S_i = sum_j exp(e_ij - M_i).

THE BOUND on |evaluation - exact value| of ONE float64 evaluation of it, u = 2^-53 (`oracle_log_density` returns it next to
the value; `exp_ulp`, `log_ulp` are the largest errors of the evaluation's exp and log in ulps of their results, `depth` the
additions a term of S goes through).  The exact value is that of the formula at the float64 numbers diff (after the wrap), W,
log_w, log_norm and log W_tot's arguments.
  diff   the difference of two float32 values is exact in float64.  A wrapped entry takes two roundings, of t + pi and of
         m - pi: |d diff_c| <= u (|t| + 2 pi), t the raw difference (both sides do the same operations, and fmod is exact, so this
         term is slack between them; it is kept because the formula's wrap is itself a float64 function).
  u_r    r + 1 multiply-adds, fused or not: |d u_r| <= (r + 1) u A_r + sum_c |W_rc| |d diff_c| =: D_r, A_r = sum_c |W_rc diff_c|
         -- with ABSOLUTE values, because the triangular product can cancel.
  q      q = sum_r u_r^2 by d multiply-adds of non-negative terms: |d q| <= sum_r (2 |u_r| D_r + D_r^2) + d u q.
  e      one multiply-add: |d e| <= 1/2 |d q| + u |e|.
  M      a max is exact: M is the largest COMPUTED e.  The formula's value does not depend on the shift, so M is taken as an
         exact number and its only error is that of the e it came from, which is counted in that term's exponent.
  a_j    the exponent e_j - M, one rounding: |d a_j| <= |d e_j| + u |a_j| =: eta_j.
  exp    t_j = exp(a_j) with relative error expm1(eta_j) from the exponent and 2 u exp_ulp from the function (an ulp of y is
         at most 2 u y): rho_j = expm1(eta_j) + 2 u exp_ulp.
  S      a sum of non-negative terms: |d S| / S <= theta = sum_j t_j rho_j / S + depth u.  (Far samples have a large eta_j
         and a negligible t_j: the average is weighted by the terms.)
  log    |d log S| <= theta (1 + theta) + 2 u log_ulp |log S|.
  W_tot  log n (unweighted): 2 u log_ulp |log n|; log_w_sum itself (weighted): 0; under exclude_self with weights
         log(exp(log_w_sum) - exp(log_w_i)): ((E1 + E2) 2 u exp_ulp + u (E1 - E2)) / (E1 - E2) + 2 u log_ulp |log|.
  +      three final additions: u (|log_norm + M| + |log_norm + M + log S| + |result|).
Everything on the right-hand sides is evaluated from the oracle's float64 numbers and multiplied by 1 + 1e-6 for their own
roundings.  A query whose every e is -inf has value -inf and bound 0; a NaN stays a NaN.
For the numpy oracle itself exp_ulp = log_ulp = 1 (glibc's exp and log are within one ulp) and depth = n, which bounds a sum
in any order.

AGAINST SCIPY.  gaussian_kde.logpdf is another float64 evaluation of the same value, so the bound is taken twice, once for
each evaluation, and multiplied by cond(H), the 2-norm condition number the test computes: scipy's triangular solves lose up
to that many roundings.  But scipy's evaluation is not the formula's: it whitens the samples and the queries FIRST
(solve_triangular of the points, scipy/stats/_stats.pyx gaussian_kernel_estimate_log) and subtracts afterwards, so "diff is
exact" does not hold for it -- the difference of two whitened coordinates of size |W| |x| cancels, and its error is
(r + 1) u sum_c |W_rc| (|x_jc| + |q_ic|), not (r + 1) u sum_c |W_rc diff_c|.  With points tens of metres from the origin and
bandwidths of decimetres that is the largest term by far: on the 1-D case here (|x| / h = 260, cond(H) = 1) scipy is 1.2e-13
from the 50-digit value where the oracle is 7e-16 from it and twice the oracle's own bound is 3e-14.  So the scipy evaluation's
share of the bound is the derivation above with A_r = sum_c |W_rc| (|x_jc| + |q_ic|) (`whitened_points`), and the check is
    |oracle - scipy| <= (bound(oracle) + bound(whitened points)) x cond(H),
while the oracle itself is held to its own bound against mpmath on the same queries, with no factor.

AGAINST scipy's covariance: `density_bandwidth` is one division and one multiplication of the population covariance, which
the test forms in float64 in another order than numpy's cov; 8 u relative per entry, times the condition number of the
covariance (an off-diagonal entry is a sum with cancellation)."""
import ctypes as C
import math
import os

import mpmath
import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from utils import Statistics as ST

U = 2.0 ** -53
PI, TWO_PI = 3.141592653589793238462643383279, 6.283185307179586476925286766559
SLACK = 1.0 + 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = dict(np.load(os.path.join(GOLDEN, "sample_density.npz"), allow_pickle=False))
    return _fixture


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def wrap_pi_near(t):
    """sample_common.h's wrap_pi_near in float64: (t + pi) mod 2 pi - pi, fmod only where t + pi leaves [0, 2 pi)."""
    with np.errstate(invalid="ignore"):
        m = t + PI
        r = np.fmod(m, TWO_PI)
        r = np.where(r < 0.0, r + TWO_PI, r)
        return np.where((m >= 0.0) & (m < TWO_PI), m, r) - PI


def log_norm_of(W):
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    return float(np.log(np.diag(W)).sum() - 0.5 * W.shape[0] * np.log(2.0 * np.pi))


def oracle_energies(q, x, qcols, xcols, W, wrap=None, log_w=None, whitened_points=False):
    """-> (diff [m, n, d] float64 after the wrap, e [m, n], de [m, n]: the bound of the head comment on one float64 evaluation
    of e) for the float32 queries q [m, *] and samples x [n, *].  `whitened_points`: the bound of an evaluation that whitens
    samples and queries first and subtracts afterwards (scipy's), A_r = sum_c |W_rc| (|x_jc| + |q_ic|)."""
    q, x = np.asarray(q, dtype=np.float32), np.asarray(x, dtype=np.float32)
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    d = len(qcols)
    m, n = q.shape[0], x.shape[0]
    diff, ddiff, mag = np.zeros((m, n, d)), np.zeros((m, n, d)), np.zeros((m, n, d))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(d):
            t = x[:, xcols[c]].astype(np.float64)[None, :] - q[:, qcols[c]].astype(np.float64)[:, None]
            mag[:, :, c] = np.abs(x[:, xcols[c]].astype(np.float64))[None, :] + np.abs(q[:, qcols[c]].astype(np.float64))[:, None]
            if wrap is not None and wrap[c]:
                ddiff[:, :, c] = U * (np.abs(t) + TWO_PI)
                t = wrap_pi_near(t)
            diff[:, :, c] = t
        qq, dqq = np.zeros((m, n)), np.zeros((m, n))
        for r in range(d):
            u, A, extra = np.zeros((m, n)), np.zeros((m, n)), np.zeros((m, n))
            for c in range(r + 1):
                u = u + W[r, c] * diff[:, :, c]
                A = A + (abs(W[r, c]) * mag[:, :, c] if whitened_points else np.abs(W[r, c] * diff[:, :, c]))
                extra = extra + abs(W[r, c]) * ddiff[:, :, c]
            D = (r + 1) * U * A + extra
            qq = qq + u * u
            dqq = dqq + 2.0 * np.abs(u) * D + D * D
        dqq = dqq + d * U * qq
        lw = np.zeros(n) if log_w is None else np.asarray(log_w, dtype=np.float64)
        e = -0.5 * qq + lw[None, :]
        de = 0.5 * dqq + U * np.where(np.isfinite(e), np.abs(e), 0.0)
    return diff, e, de * SLACK


def oracle_log_density(q, x, qcols, xcols, W, wrap=None, log_w=None, log_w_sum=None, exclude_self=False, exp_ulp=1.0, log_ulp=1.0,
                       depth=None, log_norm=None, whitened_points=False):
    """The formula of the head comment in float64 numpy -> (log_dens [m], bound [m]): the value and how far ONE float64
    evaluation with the given ulp figures and sum depth (default: n, any order) may lie from the exact value."""
    diff, e, de = oracle_energies(q, x, qcols, xcols, W, wrap, log_w, whitened_points)
    m, n = e.shape
    depth = n if depth is None else depth
    log_norm = log_norm_of(W) if log_norm is None else log_norm
    if exclude_self:
        assert m == n
        e = e.copy()
        e[np.arange(n), np.arange(n)] = -np.inf
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        M = np.max(e, axis=1)                                       # (np.max hands a NaN on)
        dead = M == -np.inf
        a = e - np.where(dead, 0.0, M)[:, None]
        t = np.exp(a)
        S = np.array([math.fsum(row) for row in np.where(np.isnan(t), 0.0, t)]) + np.where(np.isnan(t).any(axis=1), np.nan, 0.0)
        eta = de + U * np.where(np.isfinite(a), np.abs(a), 0.0)
        rho = np.expm1(eta) + 2.0 * U * exp_ulp
        theta = np.where(t > 0, t * rho, 0.0).sum(axis=1) / S + depth * U
        logS = np.log(S)
        err = theta * (1.0 + theta) + 2.0 * U * log_ulp * np.abs(logS)
        if log_w is None:
            L = np.full(m, np.log(float(n - (1 if exclude_self else 0))) if n - (1 if exclude_self else 0) > 0 else -np.inf)
            dL = 2.0 * U * log_ulp * np.abs(L)
        elif not exclude_self:
            L, dL = np.full(m, float(log_w_sum)), np.zeros(m)
        else:
            E1, E2 = np.exp(float(log_w_sum)), np.exp(np.asarray(log_w, dtype=np.float64))
            L = np.log(E1 - E2)
            dL = ((E1 + E2) * 2.0 * U * exp_ulp + U * (E1 - E2)) / (E1 - E2) + 2.0 * U * log_ulp * np.abs(L)
        p1 = log_norm + M
        p2 = p1 + logS
        value = p2 - L
        bound = (err + dL + U * (np.abs(p1) + np.abs(p2) + np.abs(value))) * SLACK
        value = np.where(dead, -np.inf, value)
        bound = np.where(dead, 0.0, bound)
    return value, bound


def mp_log_density(q, x, qcols, xcols, W, wrap=None, log_w=None, log_w_sum=None, exclude_self=False, log_norm=None):
    """The same formula in mpmath at 50 digits, from the same float64 numbers (the wrapped differences of `oracle_energies`, W,
    log_w, log_norm, log_w_sum) -> list of mpf (-inf for a query to which nothing contributes)."""
    diff, e64, _ = oracle_energies(q, x, qcols, xcols, W, wrap, log_w)
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    m, n, d = diff.shape
    log_norm = log_norm_of(W) if log_norm is None else log_norm
    out = []
    with mpmath.workdps(50):
        Wm = [[mpmath.mpf(float(W[r, c])) for c in range(r + 1)] for r in range(d)]
        lw = [mpmath.mpf(0)] * n if log_w is None else [mpmath.mpf(float(v)) if np.isfinite(v) else None for v in log_w]
        half = mpmath.mpf(0.5)
        for i in range(m):
            es = []
            for j in range(n):
                if (exclude_self and i == j) or lw[j] is None:
                    continue
                dm = [mpmath.mpf(float(v)) for v in diff[i, j]]
                qq = mpmath.mpf(0)
                for r in range(d):
                    u = mpmath.fsum(Wm[r][c] * dm[c] for c in range(r + 1))
                    qq += u * u
                es.append(lw[j] - half * qq)
            if not es:
                out.append(mpmath.mpf("-inf"))
                continue
            M = max(es)
            S = mpmath.fsum(mpmath.exp(v - M) for v in es)
            if log_w is None:
                L = mpmath.log(n - (1 if exclude_self else 0))
            elif not exclude_self:
                L = mpmath.mpf(float(log_w_sum))
            else:
                L = mpmath.log(mpmath.exp(mpmath.mpf(float(log_w_sum))) - mpmath.exp(mpmath.mpf(float(log_w[i]))))
            out.append(mpmath.mpf(float(log_norm)) + M + mpmath.log(S) - L)
    return out


def mp_errors(values, exact):
    """|value - exact| per query as floats (0 where both are -inf)."""
    out = []
    with mpmath.workdps(50):
        for v, ex in zip(values, exact):
            if ex == mpmath.mpf("-inf"):
                out.append(0.0 if v == -np.inf else np.inf)
            else:
                out.append(float(abs(mpmath.mpf(float(v)) - ex)) if np.isfinite(v) else np.inf)
    return np.array(out)


# ---- sample sets for the tests (the GPU tests use them too) --------------------------------------------------------------------
POSE_WRAP = np.array([0, 0, 1, 0, 0, 1], dtype=np.uint8)


def cloud(n, seed, spread=1.0):
    """[n, 6] float32: two SE(2) poses -- correlated xy offset by tens of metres, headings that straddle the +-pi seam."""
    rng = np.random.RandomState(seed)
    A = np.tril(rng.normal(size=(6, 6))) * 0.6 + np.eye(6)
    z = rng.normal(size=(n, 6)) @ A.T * spread
    z[:, [2, 5]] *= 0.4
    z += np.array([37.5, -62.25, 3.0, 18.0, 91.0, -3.1])
    z[:, [2, 5]] = np.mod(z[:, [2, 5]] + np.pi, 2 * np.pi) - np.pi
    return z.astype(np.float32)


def fixed_whiten(d, seed=3):
    """A lower-triangular W [d, d] = inv(L) that does not depend on the samples (so that n = 1 has one): L has off-diagonal
    entries, a diagonal in 0.4 .. 0.9, and heading rows (2, 5) scaled by 0.5: their kernel width L_rr is under pi / 3."""
    rng = np.random.RandomState(seed + d)
    L = np.tril(rng.normal(size=(d, d)), -1) * 0.3 + np.diag(rng.uniform(0.4, 0.9, d))
    for r in (2, 5):
        if r < d:
            L[r] *= 0.5
    return np.tril(np.linalg.solve(L, np.eye(d)))


def population_covariance(x, w=None):
    x = np.asarray(x, dtype=np.float64)
    w = np.ones(x.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
    mean = (w[:, None] * x).sum(axis=0) / w.sum()
    r = x - mean
    return (w[:, None, None] * r[:, :, None] * r[:, None, :]).sum(axis=0) / w.sum()


def oracle_loo_scores(x, factors, w=None):
    """The (weighted) mean leave-one-out log density of the 1-D set x under every bandwidth factor -> (scores, bounds)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 1)
    n = x.shape[0]
    n_eff = ST.effective_sample_size(w, n)
    cov = population_covariance(x, w)
    scores, bounds = [], []
    lw = None if w is None else np.log(w)
    for f in factors:
        W = ST.density_whiten(ST.density_bandwidth(cov, n_eff, 1, float(f)))
        v, b = oracle_log_density(x, x, [0], [0], W, None, lw, None if w is None else float(np.log(w.sum())), True)
        ww = np.ones(n) if w is None else w
        scores.append(float((ww * v).sum() / ww.sum()))
        bounds.append(float((ww * b).sum() / ww.sum() + (n + 2) * U * (ww * np.abs(v)).sum() / ww.sum()))
    return np.array(scores), np.array(bounds)


def loo_factors(n_eff, d=1):
    return np.array([ST.density_factor(n_eff, d, "scott") * 2.0 ** (k / 2.0) for k in ST.DENSITY_LOO_POWERS])


# ---- 1. the oracle against mpmath and against scipy --------------------------------------------------------------------------------
@pytest.mark.parametrize("d, n, m", [(1, 1, 3), (2, 33, 9), (3, 40, 7), (6, 30, 5)])
def test_oracle_against_mpmath(d, n, m):
    x, q = cloud(n, 10 + d), cloud(m, 20 + d, spread=2.0)
    q[0] = x[0]
    q[-1, :2] += 4000.0                                             # thousands of bandwidths away
    cols = list(range(d))
    W = fixed_whiten(d)
    w = np.random.RandomState(d).uniform(0.1, 2.0, n)
    if n > 2:
        w[1] = 0.0
    with np.errstate(divide="ignore"):
        lw = np.log(w)
    for kw in (dict(), dict(log_w=lw, log_w_sum=float(np.log(w.sum())))):
        v, b = oracle_log_density(q, x, cols, cols, W, POSE_WRAP[:d], **kw)
        err = mp_errors(v, mp_log_density(q, x, cols, cols, W, POSE_WRAP[:d], **kw))
        print(d, n, "weighted" if kw else "plain", "worst error / bound", np.max(err / b))
        assert np.all(np.isfinite(v)) and np.all(err <= b)
    if n > 1:
        for kw in (dict(), dict(log_w=lw, log_w_sum=float(np.log(w.sum())))):
            v, b = oracle_log_density(x, x, cols, cols, W, POSE_WRAP[:d], exclude_self=True, **kw)
            err = mp_errors(v, mp_log_density(x, x, cols, cols, W, POSE_WRAP[:d], exclude_self=True, **kw))
            assert np.all(err <= b), np.max(err / np.maximum(b, 1e-300))
    else:
        v, b = oracle_log_density(x, x, cols, cols, W, None, exclude_self=True)
        assert v[0] == -np.inf and b[0] == 0.0
    far, _ = oracle_log_density(q[-1:], x, cols, cols, W, POSE_WRAP[:d])
    assert np.isfinite(far[0]) and far[0] < -1e6 and np.exp(far[0]) == 0.0


def test_oracle_special_cases():
    x = cloud(5, 1)
    W = fixed_whiten(3)
    q = x[:3].copy()
    q[1, 1] = np.nan
    v, _ = oracle_log_density(q, x, [0, 1, 2], [0, 1, 2], W, POSE_WRAP[:3])
    assert np.isnan(v[1]) and np.isfinite(v[[0, 2]]).all()
    lw = np.full(5, -np.inf)
    v, b = oracle_log_density(q[:1], x, [0], [0], W[:1, :1], None, lw, 0.0)
    assert v[0] == -np.inf and b[0] == 0.0
    # the seam: samples at +-(pi - 0.01), a query at pi - 0.005; wrapped, both samples are near; unwrapped, one is 2 pi away
    s = np.array([[np.pi - 0.01], [-(np.pi - 0.01)]], dtype=np.float32)
    p = np.array([[np.pi - 0.005]], dtype=np.float32)
    Wh = np.array([[1.0 / 0.05]])
    wrapped, _ = oracle_log_density(p, s, [0], [0], Wh, [1])
    plain, _ = oracle_log_density(p, s, [0], [0], Wh, [0])
    assert wrapped[0] > plain[0] + 0.3 and abs(plain[0] - (log_norm_of(Wh) - 0.5 * (0.005 / 0.05) ** 2 - np.log(2))) < 1e-4


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("rule", ["scott", "silverman"])
def test_bandwidth_and_oracle_against_scipy(k, rule):
    fx = fixture()
    x, q = fx["x%d" % k], fx["q%d" % k]
    w = fx["w%d" % k] if "w%d" % k in fx else None
    n, d = x.shape
    n_eff = ST.effective_sample_size(w, n)
    assert abs(n_eff - float(fx["neff%d" % k])) <= 8 * U * n_eff
    cov = population_covariance(x, w)
    H = ST.density_bandwidth(cov, n_eff, d, rule)
    ref = fx["cov_%s%d" % (rule, k)]
    cond = float(np.linalg.cond(ref))
    rel = np.max(np.abs(H - ref) / np.abs(ref))
    print("case", k, rule, "bandwidth: relative error", rel, "condition number", cond)
    assert rel <= 8 * U * cond
    W = ST.density_whiten(H)
    assert np.allclose(W @ H @ W.T, np.eye(d), rtol=0, atol=1e-9 * cond) and np.all(np.triu(W, 1) == 0)
    cols = list(range(d))
    kw = dict()
    if w is not None:
        with np.errstate(divide="ignore"):
            kw = dict(log_w=np.log(w), log_w_sum=float(np.log(w.sum())))
    v, b = oracle_log_density(q, x, cols, cols, W, None, **kw)
    _, b_scipy = oracle_log_density(q, x, cols, cols, W, None, whitened_points=True, **kw)
    ref = fx["logpdf_%s%d" % (rule, k)]
    err = np.abs(v - ref)
    print("case", k, rule, "oracle against scipy: worst |d log|", err.max(), "where the log is", ref[np.argmax(err)],
          "worst error / bound", np.max(err / ((b + b_scipy) * cond)), "(against twice the oracle's own bound x cond:",
          np.max(err / (2.0 * b * cond)), ")")
    assert np.all(err <= (b + b_scipy) * cond)
    pick = np.argsort(-err / b)[:12]                                # the oracle itself, where it is furthest from scipy: no factor
    own = mp_errors(v[pick], mp_log_density(q[pick], x, cols, cols, W, None, **kw))
    print("case", k, rule, "oracle against mpmath there: worst error / bound", np.max(own / b[pick]))
    assert np.all(own <= b[pick])
    assert ref.min() < -1e6                                         # the tails are part of the check


# ---- 2. the host statistics --------------------------------------------------------------------------------------------------------
def test_density_factor_and_bandwidth_rules():
    assert ST.density_factor(100.0, 1, "scott") == 100.0 ** (-1.0 / 5.0)
    assert ST.density_factor(100.0, 2, "silverman") == (100.0 * 4.0 / 4.0) ** (-1.0 / 6.0)
    assert ST.density_factor(7.0, 3, 0.25) == 0.25
    cov = np.array([[3.0, 0.5], [0.5, 6.0]])
    H = ST.density_bandwidth(cov, 50.0, 2, 0.5)
    assert np.allclose(H, cov / (1 - 1 / 50.0) * 0.25, rtol=4 * U, atol=0)
    # a circular column's variance is capped at pi^2 / 3 before the factor: row and column shrink together
    Hc = ST.density_bandwidth(cov, 50.0, 2, 0.5, circular=[False, True])
    s = np.sqrt(np.pi ** 2 / 3 / 6.0)
    assert np.allclose(Hc, np.array([[3.0, 0.5 * s], [0.5 * s, np.pi ** 2 / 3]]) / (1 - 1 / 50.0) * 0.25, rtol=8 * U, atol=0)
    assert np.array_equal(ST.density_bandwidth(cov, 50.0, 2, 0.5, circular=[True, False]), H)      # 3 < pi^2 / 3: untouched
    ring = ST.density_bandwidth([[3.2]], 200.0, 1, "scott", circular=[True])
    assert np.sqrt(ring[0, 0]) < np.pi / 3
    for bad, match in (((np.array([[1.0, 0], [0, 0.0]]), 50.0, 2, "scott"), "no spread"),
                       ((np.array([[1.0, 0], [0, np.nan]]), 50.0, 2, "scott"), "no spread"),
                       ((cov, 1.0, 2, "scott"), "above 1"), ((cov, 50.0, 2, "scot"), "bandwidth is"),
                       ((cov, 50.0, 2, -1.0), "bandwidth is"), ((cov, 50.0, 2, 0.0), "bandwidth is"),
                       ((cov, 50.0, 2, np.inf), "bandwidth is"), ((cov, 50.0, 2, True), "bandwidth is")):
        with pytest.raises(ValueError, match=match):
            ST.density_bandwidth(*bad)
    with pytest.raises(ValueError, match="positive definite"):
        ST.density_whiten(np.array([[1.0, 1.0], [1.0, 1.0]]))
    for bw in ("scott", "silverman", "loo", 0.3):
        ST.check_density_options(bw, 2)
    for args, match in ((("scot", 5), "bandwidth is"), ((-0.5, 5), "bandwidth is"), (("scott", 1), "at least two samples"),
                        (("scott", 5, 4, True), "exclude_self")):
        with pytest.raises(ValueError, match=match):
            ST.check_density_options(*args)


def test_hpd_level():
    s = np.array([-1.0, -2.0, -3.0, -4.0])
    assert ST.hpd_level(s, -2.5) == 0.5 and ST.hpd_level(s, -0.5) == 0.0 and ST.hpd_level(s, -9.0) == 1.0
    assert ST.hpd_level(s, -2.0) == 0.5                             # "at least": the sample of equal density counts
    assert ST.hpd_level(s, -2.5, weights=[3.0, 1.0, 0.0, 4.0]) == 0.5
    assert np.array_equal(ST.hpd_level(s, np.array([-0.5, -3.5])), [0.0, 0.75])
    t = ST.hpd_level(torch.from_numpy(s), torch.tensor([-0.5, -3.5], dtype=torch.float64), torch.tensor([1.0, 1.0, 2.0, 0.0]))
    assert torch.is_tensor(t) and t.tolist() == [0.0, 1.0]
    assert float(ST.hpd_level(torch.from_numpy(s), -2.5)) == 0.5
    # on the oracle: the level of a Gaussian sample's own mean is small, that of a point in the tail is 1
    x = np.random.RandomState(4).normal(size=(400, 1)).astype(np.float32)
    W = ST.density_whiten(ST.density_bandwidth(population_covariance(x), 400.0, 1, "scott"))
    own, _ = oracle_log_density(x, x, [0], [0], W)
    at, _ = oracle_log_density(np.array([[0.0], [1.0], [6.0]], dtype=np.float32), x, [0], [0], W)
    lev = ST.hpd_level(own, at)
    print("hpd levels at 0, 1, 6 sigma:", lev)
    assert lev[0] < 0.2 and 0.55 < lev[1] < 0.8 and lev[2] == 1.0     # (exactly 0, 0.683, 1 for the Gaussian itself)


def test_leave_one_out_selection_on_the_bimodal_set():
    """Half N(-5, 0.3^2), half N(5, 0.3^2): Scott's rule gives h = 1.45 against a mode width of 0.3; the leave-one-out rule
    picks 2^-4 of it, h = 0.09, and the mean leave-one-out log density is -0.86 against -2.02.  The best two scores are 50
    bounds or more apart (2.7e-3 against bounds of 1e-13): the GPU test's selection excuses no tie."""
    x = fixture()["bimodal"]
    assert x.shape == (500,) and x.dtype == np.float32
    factors = loo_factors(500.0)
    scott = ST.density_factor(500.0, 1, "scott")
    h = np.sqrt(ST.density_bandwidth(population_covariance(x.reshape(-1, 1)), 500.0, 1, "scott")[0, 0])
    scores, bounds = oracle_loo_scores(x, factors)
    best = int(np.argmax(scores))
    print("scott h", h, "scores", scores, "picked power", ST.DENSITY_LOO_POWERS[best], "h", h * factors[best] / scott)
    assert abs(h - 1.45) < 0.01
    assert ST.DENSITY_LOO_POWERS[best] == -8 and abs(h * factors[best] / scott - 0.09) < 0.005
    at_scott = scores[list(ST.DENSITY_LOO_POWERS).index(0)]
    print("mean leave-one-out log density:", scores[best], "against Scott's", at_scott)
    assert scores[best] > at_scott + 1.0                            # more than a nat per sample
    order = np.argsort(-scores)
    gap = scores[order[0]] - scores[order[1]]
    print("best two scores differ by", gap, "bounds", bounds[order[:2]])
    assert gap >= 50.0 * (bounds[order[0]] + bounds[order[1]])


# ---- 3. the binding's tables and refusals ------------------------------------------------------------------------------------------
def test_pack_and_check_density_blocks():
    W2, W1 = fixed_whiten(2), np.array([[4.0]])
    t = nh.pack_density_blocks([2, 1], [W2, W1])
    assert t.dtype == nh.DENSITY_BLOCK_DTYPE and t.dtype.itemsize == 184 == C.sizeof(nh.DensityBlock)
    assert t["col_off"].tolist() == [0, 2] and t["d"].tolist() == [2, 1]
    assert t["whiten"][0, :3].tolist() == [W2[0, 0], W2[1, 0], W2[1, 1]] and not t["whiten"][0, 3:].any()
    assert t["log_norm"][0] == log_norm_of(W2) and t["log_norm"][1] == np.log(4.0) - 0.5 * np.log(2 * np.pi)
    W6 = fixed_whiten(6)
    t6 = nh.pack_density_blocks([6, 6], [W6, W6], col_off=[0, 0])
    assert t6["col_off"].tolist() == [0, 0] and np.array_equal(t6["whiten"][1], W6[np.tril_indices(6)])
    nh.check_density_blocks(t, [0, 1, 2], [2, 1, 0], 3, 3, [0, 0, 1])
    nh.check_density_blocks(t6, np.arange(6), np.arange(6), 6, 6, POSE_WRAP)
    for dims, mats, match in (([7], [np.eye(7)], "d in 1..6"), ([2], [np.eye(3)], "d in 1..6"), ([2, 1], [W2], "one whitening matrix")):
        with pytest.raises(ValueError, match=match):
            nh.pack_density_blocks(dims, mats)

    def bad(field, value, row=0):
        b = t.copy()
        if isinstance(field, tuple):
            b[field[0]][row, field[1]] = value
        else:
            b[field][row] = value
        return b

    cases = [(bad("d", 0), "width 0"), (bad("d", 7), "width 7"), (bad("col_off", 2), "leave"), (bad("col_off", -1), "leave"),
             (bad("log_norm", np.inf), "finite"), (bad(("whiten", 1), np.nan), "finite"), (bad(("whiten", 2), 0.0), "positive diagonal"),
             (bad(("whiten", 0), -1.0), "positive diagonal"), (t.astype(nh.DENSITY_BLOCK_DTYPE)[:0], "1..65535 blocks"),
             (np.zeros(2, dtype=nh.KNN_BLOCK_DTYPE), "DENSITY_BLOCK_DTYPE")]
    for table, match in cases:
        with pytest.raises(ValueError, match=match):
            nh.check_density_blocks(table, [0, 1, 2], [0, 1, 2], 3, 3, None)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_density_blocks(t, [0, 1, 3], [0, 1, 2], 3, 3)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_density_blocks(t, [0, 1, 2], [0, -1, 2], 3, 3)
    with pytest.raises(ValueError, match="same length"):
        nh.check_density_blocks(t, [0, 1, 2], [0, 1], 3, 3)
    with pytest.raises(ValueError, match="one value per entry"):
        nh.check_density_blocks(t, [0, 1, 2], [0, 1, 2], 3, 3, [0, 1])
    # the pi / 3 rule: a circular entry's kernel width 1 / W_rr
    wide = nh.pack_density_blocks([1], [np.array([[1.0 / 1.2]])])
    nh.check_density_blocks(wide, [0], [0], 1, 1, [0])
    with pytest.raises(ValueError, match="pi / 3"):
        nh.check_density_blocks(wide, [0], [0], 1, 1, [1])
    nh.check_density_blocks(nh.pack_density_blocks([1], [np.array([[1.0 / 1.04]])]), [0], [0], 1, 1, [1])
    for args, match in (((0, 5), "at least one point"), ((5, 0), "at least one point"), ((5, 6, True), "exclude_self"),
                        ((65535 * 64 + 1, 5), "out of range")):
        with pytest.raises(ValueError, match=match):
            nh.check_density_args(*args)


def test_host_side_refusals_of_the_c_entry():
    """The entry refuses bad arguments on the host, before it touches the device (the pointers below are never dereferenced:
    they are not device memory)."""
    nh.build()
    lib = nh.lib()
    assert lib.nfisam_abi_version() == 1600
    blocks = nh.pack_density_blocks([2, 3], [fixed_whiten(2), fixed_whiten(3)])
    fake = C.c_void_p(4096)

    def call(Qt=fake, qr=4, m=5, Xt=fake, xr=4, n=5, ex=0, blk=blocks, blk_dev=fake, nb=2, qc=fake, xc=fake, ne=5, log_w=None,
             lws=0.0, out=fake):
        return lib.nfisam_sample_density(Qt, qr, m, Xt, xr, n, ex, None if blk is None else blk.ctypes.data_as(C.c_void_p), blk_dev,
                                         nb, qc, xc, ne, None, log_w, C.c_double(lws), out, None, None)

    for kw in [dict(Qt=None), dict(Xt=None), dict(blk=None), dict(blk_dev=None), dict(qc=None), dict(xc=None), dict(out=None),
               dict(m=0), dict(n=0), dict(m=-1), dict(qr=0), dict(xr=0), dict(ne=0), dict(nb=0), dict(nb=65536),
               dict(m=65535 * 64 + 1), dict(ex=1, n=6), dict(log_w=fake, lws=float("nan")), dict(log_w=fake, lws=float("inf"))]:
        assert call(**kw) == nh.ERR_ARG, kw
    for field, at, value in (("d", None, 0), ("d", None, 7), ("d", None, -1), ("log_norm", None, np.nan), ("log_norm", None, np.inf),
                             ("whiten", 1, np.nan), ("whiten", 3, np.inf), ("whiten", 2, 0.0), ("whiten", 5, -1.0)):
        bad = blocks.copy()
        if at is None:
            bad[field][1] = value
        else:
            bad[field][1, at] = value
        assert call(blk=bad) == nh.ERR_ARG, (field, at, value)
    junk = blocks.copy()
    junk["whiten"][0, 3:] = np.nan                                  # beyond d (d + 1) / 2: not read
    bad = junk.copy()
    bad["d"][0] = 7
    assert call(blk=bad) == nh.ERR_ARG
    assert "nfisam_sample_density" in nh.EXPORTS and hasattr(lib, "nfisam_sample_density")
    hdr = open(nh.CSRC + "/../../include/nfisam_hip.h").read()
    assert "int nfisam_sample_density(" in hdr and "} nfisam_density_block;" in hdr and "#define NFISAM_DENSITY_MAX_D 6" in hdr
    assert nh.DENSITY_MAX_D == 6
    assert "sample_density" in open(nh.CSRC + "/Makefile").read() and "sample_density.hip" in open(nh.CSRC + "/sample_common.h").read()
    assert "sample_density.hip" in open(nh.CSRC + "/sample_pairs.h").read()


class Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


def test_cpu_tensors_are_refused_and_nothing_is_uploaded(monkeypatch):
    refuse = Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    t = nh.pack_density_blocks([2], [fixed_whiten(2)])
    X = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_density(X, None, t, [0, 1], [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_density(X.numpy(), X.numpy(), t, [0, 1], [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_density_t(X.t().contiguous(), None, t, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="out of range"):
        nh.sample_density(X.numpy(), None, t, [0, 3], [0, 1], device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        nh.sample_density(X.numpy(), X.numpy()[:, :1], t, [0, 1], [0, 1], device="cuda")
    with pytest.raises(ValueError, match="exclude_self"):
        nh.sample_density(X.numpy(), X.numpy()[:4], t, [0, 1], [0, 1], exclude_self=True, device="cuda")
    with pytest.raises(ValueError, match="at least one point"):
        nh.sample_density(X.numpy()[:0], X.numpy(), t, [0, 1], [0, 1], device="cuda")
    with pytest.raises(ValueError, match="pi / 3"):
        nh.sample_density(X.numpy(), None, nh.pack_density_blocks([1], [np.array([[0.5]])]), [2], [2], wrap=[1], device="cuda")
    for w, match in ((np.ones(4), "weights must be"), (-np.ones(5), "non-negative"), (np.zeros(5), "not all zero")):
        with pytest.raises(ValueError, match=match):
            nh.sample_density(X.numpy(), None, t, [0, 1], [0, 1], weights=w, device="cuda")
    assert refuse.calls == 0


@pytest.mark.parametrize("kwargs, match", [
    (dict(bandwidth="scot"), "bandwidth is"), (dict(bandwidth=-1.0), "bandwidth is"), (dict(bandwidth=0), "bandwidth is"),
    (dict(blocks=[]), "no blocks"), (dict(blocks=[[0, 3]]), "outside its matrix"), (dict(blocks=[list(range(7))]), "at most 6"),
    (dict(blocks=[([0, 1], [0])]), "equal length"), (dict(circular=[True]), "circular"), (dict(weights=np.ones(3)), "weights must be"),
    (dict(weights=-np.ones(8)), "non-negative"), (dict(exclude_self=True, queries=np.zeros((5, 3), dtype=np.float32)), "exclude_self"),
    (dict(queries=np.zeros(5)), "queries must be"), (dict(queries=np.zeros((0, 3), dtype=np.float32)), "no queries"),
    (dict(queries=np.zeros((4, 2), dtype=np.float32), blocks=[[0, 2]]), "outside its matrix"),
])
def test_statistics_refuse_before_any_launch(monkeypatch, kwargs, match):
    refuse = Refuse()
    for name in ("upload", "sample_density_t", "sample_moments_t", "_columns"):
        monkeypatch.setattr(nh, name, refuse)
    kw = dict(kwargs)
    x = np.zeros((8, 3), dtype=np.float32)
    queries = kw.pop("queries", None)
    blocks = kw.pop("blocks", [[0, 1], [2]])
    with pytest.raises(ValueError, match=match):
        ST.sample_density(x, queries, blocks, device="cuda", **kw)
    with pytest.raises(ValueError, match="points, columns"):
        ST.sample_density(np.zeros(8), None, [[0]], device="cuda")
    with pytest.raises(ValueError, match="at least two samples"):
        ST.sample_density(x[:1], None, [[0]], device="cuda")
    assert refuse.calls == 0


def test_posterior_marginal_density_errors_come_before_any_launch(monkeypatch):
    """On a solver whose graph is a pose prior and a range factor over {X0, L1}, eliminated but never trained."""
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_marginal_density is NFiSAM.posterior_marginal_density
    nh.build()
    with pytest.raises(RuntimeError, match="posterior_marginal_density: no factor graph"):
        NFiSAM().posterior_marginal_density(curves=10)
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    s.add_node(X0)
    s.add_node(L1)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    refuse = Refuse()
    for name in ("sample_moments", "sample_moments_t", "sample_density", "sample_density_t", "posterior_walk_raw", "upload", "_columns",
                 "density_log_weights"):
        monkeypatch.setattr(nh, name, refuse)
    X9 = SE2Variable("X9")
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    what = "posterior_marginal_density: "
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):
        s.posterior_marginal_density(curves=10)
    for kw, match in [
            (dict(), what + "ask for at least one"), (dict(curves=1), "curves is the number"), (dict(curves=2.5), "curves is the number"),
            (dict(curves=True), "curves is the number"), (dict(maps=(1, 4)), "maps is"), (dict(maps=8), "maps is"), (dict(maps=(4, 4, 4)), "maps is"),
            (dict(maps=(4, 4), variables=[]), "no variable"), (dict(curves=5, variables=[X0, X9]), "X9 is not in the elimination ordering"),
            (dict(curves=5, pairs=[(X0, X9)]), "X9 is not in the elimination ordering"), (dict(curves=5, pairs=[(X0, L1, X0)]), "pair"),
            (dict(curves=5, bandwidth="scot"), what + "bandwidth is"), (dict(curves=5, bandwidth=-2.0), what + "bandwidth is"),
            (dict(curves=5, weights=np.ones(6)), what + "weights must be"), (dict(curves=5, weights="importanse"), "weights is None"),
            (dict(at={X9: np.zeros((2, 3))}), "not among the variables and pairs"), (dict(at={(X0, L1): np.zeros((2, 5))}), "not among"),
            (dict(at={X0: np.zeros((2, 2))}), r"at\[X0\] must be \[q >= 1, 3\]"), (dict(at={X0: np.zeros((0, 3))}), r"at\[X0\] must be"),
            (dict(at={(X0, L1): np.zeros((2, 4))}, pairs=[(X0, L1)]), r"at\[X0/L1\] must be \[q >= 1, 5\]"), (dict(at={}), "at is empty"),
            (dict(truth={X9: np.zeros(3)}), "truth holds none"), (dict(truth={X0: np.zeros(2)}), r"truth of X0 must be \[3\]"),
            (dict(truth={X0: np.array([0.0, np.nan, 0.0])}), "truth of X0")]:
        with pytest.raises(ValueError, match=match):
            s.posterior_marginal_density(own, **kw)
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_marginal_density({X0: own[X0]}, curves=5)
    with pytest.raises(ValueError, match="no points"):
        s.posterior_marginal_density({X0: own[X0][:0], L1: own[L1][:0]}, curves=5)
    with pytest.raises(ValueError, match="at least two samples"):
        s.posterior_marginal_density({X0: own[X0][:1], L1: own[L1][:1]}, curves=5)
    X7 = SE2Variable("X7")
    s7 = NFiSAM()
    for v in (X0, X7, L1):
        s7.add_node(v)
    s7.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s7.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s7.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X7, L1, 3.0, 0.5))
    s7.update_physical_and_working_graphs()
    three = {X0: np.zeros((7, 3)), X7: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    monkeypatch.setattr(nh, "DENSITY_MAX_D", 5)                     # (two poses are 6 columns, the widest there is: narrow the limit)
    with pytest.raises(ValueError, match="6 columns wide; a density block holds at most 5"):
        s7.posterior_marginal_density(three, pairs=[(X0, X7)], curves=5)
    assert refuse.calls == 0
