"""The chain diagnostics' host side (csrc/sample_chains.hip: nfisam_chain_record / nfisam_chain_finish, nfisam_hip's bindings,
utils.Statistics.blocking_tau / check_chain_options, the `record` option of metropolis_refine_t) with no device, and the float64
numpy RESTATEMENT of the two kernels -- `fold`, `record_history`, `finish` -- that tests/test_sample_chains_gpu.py grades the
device against:

  1. the restatement (streaming accumulators, the cascade as the contract writes it) against the DIRECT form from the whole
     history: reshape into blocks, var(ddof=1), half-chains;
  2. known processes: AR(1) chains against the exact expectation of every blocking level; shifted chains raise R-hat;
  3. a circular row whose values straddle the +-pi seam gives the statistics of the same deviations about 0;
  4. the conventions of `blocking_tau`: 64 pooled degrees of freedom, a block of 4 tau;
  5. bad input is refused with no device, and the C entries refuse before any launch.

THE BOUND, derived, not measured (`acc_bound`, `finish_bounds`).  An accumulator is a sum of at most T terms, each with a
handful of roundings of its own: two valid implementations of it differ by at most 4 (T + 16) 2^-53 sum |terms| (the form of
`rounding_bound` in tests/test_sample_mcmc_cpu.py).  sum |terms| is the SAME fold run on |v|: a block mean's terms are bounded
by the block mean of |v|, its square's by that squared.  A statistic is a quotient of sums of differences of accumulators; the
bound is carried through by first-order propagation -- the error of Q - R^2 / m is e(Q) + 2 |R| e(R) / m, that of a sum over
chains adds 4 (n + 16) 2^-53 sum |terms|, a quotient adds the relative errors of its parts: (sum |terms|) / |result|, the
condition number, computed here from the restatement's own values."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI, TWO_PI = np.pi, 2.0 * np.pi
U = 2.0 ** -53
NEW = ("nfisam_chain_record", "nfisam_chain_finish", "nfisam_chain_state_count")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def wrap_pi(v):
    m = np.fmod(v + PI, TWO_PI)
    m = np.where(m < 0, m + TWO_PI, m)
    return m - PI


def slots(levels):
    return 4 + 3 * (levels - 1)


def max_levels(T):
    return min(16, int(T).bit_length() - 1)


def deviations(X, center, wrap):
    """v [rows, n] float64: x - center, wrapped where wrap is set (X float32 as the kernel reads it, or float64)."""
    X = np.asarray(X, dtype=np.float64)
    c = np.zeros(X.shape[0]) if center is None else np.asarray(center, dtype=np.float64)
    v = X - c[:, None]
    if wrap is not None:
        w = np.asarray(wrap, dtype=bool)
        v[w] = wrap_pi(v[w])
    return v


def fold_values(state, v, t, T, levels):
    """The fold of the contract at index t, on state [slots, rows, n] in place, for deviations v [rows, n]."""
    w = 0 if t < T // 2 else 1
    state[w] += v
    state[2 + w] += v * v
    carry = v
    for l in range(1, levels):
        P, R, Q = state[4 + 3 * (l - 1):7 + 3 * (l - 1)]
        if not (t >> (l - 1)) & 1:
            P[...] = carry
            break
        carry = 0.5 * (P + carry)
        R += carry
        Q += carry * carry


def fold(state, X, t, T, levels, center=None, wrap=None):
    fold_values(state, deviations(X, center, wrap), t, T, levels)


def record_history(hist, levels, center=None, wrap=None):
    """hist [T, rows, n] -> (state, abs_state): the accumulators after the T folds, and the same folds of |v| (sum |terms|)."""
    T, rows, n = hist.shape
    state, abs_state = np.zeros((slots(levels), rows, n)), np.zeros((slots(levels), rows, n))
    for t in range(T):
        v = deviations(hist[t], center, wrap)
        fold_values(state, v, t, T, levels)
        fold_values(abs_state, np.abs(v), t, T, levels)
    return state, abs_state


def acc_bound(T, abs_state):
    """Two valid implementations of an accumulator differ by at most 4 (T + 16) 2^-53 sum |terms|."""
    return 4.0 * (T + 16) * U * abs_state


def _level(state, l):
    """(R_l, Q_l) [rows, n]: level 0 is the halves added up."""
    if l == 0:
        return state[0] + state[1], state[2] + state[3]
    return state[4 + 3 * (l - 1) + 1], state[4 + 3 * (l - 1) + 2]


def finish(state, T, levels, center=None, wrap=None):
    """The finish of the contract from the accumulators -> dict(mean [rows], within [rows], rhat [rows], tau [levels, rows])."""
    rows, n = state.shape[1:]
    L = T // 2
    c = np.zeros(rows) if center is None else np.asarray(center, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        R0, Q0 = _level(state, 0)
        mean = c + R0.sum(axis=1) / (n * T)
        if wrap is not None:
            w = np.asarray(wrap, dtype=bool)
            mean[w] = wrap_pi(mean[w])
        s2 = [None] * levels
        for l in range(levels):
            m = T >> l
            R, Q = _level(state, l)
            s2[l] = ((Q - R * R / m) / (m - 1)).sum(axis=1) / n
        within = s2[0]
        tau = np.stack([(2.0 ** l) * s2[l] / s2[0] for l in range(levels)])
        A1, A2 = state[0:2], state[2:4]                               # [2, rows, n]: the 2 n half-chains
        mu = A1 / L
        W = ((A2 - A1 * A1 / L) / (L - 1)).sum(axis=(0, 2)) / (2 * n) if L > 1 else np.full(rows, np.nan)
        mu_bar = mu.sum(axis=(0, 2)) / (2 * n)
        BL = ((mu - mu_bar[None, :, None]) ** 2).sum(axis=(0, 2)) / (2 * n - 1)
        rhat = np.sqrt(((L - 1) / L * W + BL) / W) if T >= 4 else np.full(rows, np.nan)
    return dict(mean=mean, within=within, rhat=rhat, tau=tau)


def finish_bounds(state, abs_state, T, levels, center=None):
    """First-order bounds on |a valid implementation - the restatement| of every statistic, from the accumulators' bounds
    `acc_bound` -> dict(mean, within, rhat, tau [levels]) of arrays [rows].  inf where a result is 0 / 0."""
    rows, n = state.shape[1:]
    L = T // 2
    e = acc_bound(T, abs_state)
    c = np.zeros(rows) if center is None else np.abs(np.asarray(center, dtype=np.float64))

    def over_chains(terms, e_terms, count, axis):                      # a sum over chains (or half-chains) in any valid order
        return e_terms.sum(axis=axis) + 4.0 * (count + 16) * U * np.abs(terms).sum(axis=axis)

    def variance(R, Q, eR, eQ, m):                                     # (Q - R^2 / m) / (m - 1) and its bound
        s2 = (Q - R * R / m) / (m - 1)
        return s2, (eQ + 2.0 * np.abs(R) * eR / m + 3.0 * U * (np.abs(Q) + R * R / m)) / (m - 1) + U * np.abs(s2)

    with np.errstate(divide="ignore", invalid="ignore"):
        R0, Q0 = _level(state, 0)
        eR0, eQ0 = e[0] + e[1] + U * np.abs(R0), e[2] + e[3] + U * np.abs(Q0)
        gm = R0.sum(axis=1) / (n * T)
        b_mean = over_chains(R0, eR0, n, 1) / (n * T) + 2.0 * U * (np.abs(gm) + c) + 4.0 * U * PI   # (+ the centre added, the wrap)
        S, eS = [], []
        for l in range(levels):
            m = T >> l
            R, Q = _level(state, l)
            eR, eQ = (eR0, eQ0) if l == 0 else (e[4 + 3 * (l - 1) + 1], e[4 + 3 * (l - 1) + 2])
            s2, e2 = variance(R, Q, eR, eQ, m)
            S.append(s2.sum(axis=1))
            eS.append(over_chains(s2, e2, n, 1))
        within = S[0] / n
        b_within = eS[0] / n + U * np.abs(within)
        b_tau = np.stack([np.abs((2.0 ** l) * S[l] / S[0]) * (eS[l] / np.abs(S[l]) + eS[0] / np.abs(S[0]) + 4.0 * U)
                          for l in range(levels)])
        b_tau[0] = 4.0 * U                                             # x / x
        if T >= 4:
            A1, A2 = state[0:2], state[2:4]
            s2, e2 = variance(A1, A2, e[0:2], e[2:4], L)
            SW, eSW = s2.sum(axis=(0, 2)), over_chains(s2, e2, 2 * n, (0, 2))
            mu, e_mu = A1 / L, e[0:2] / L + U * np.abs(A1 / L)
            mu_bar = mu.sum(axis=(0, 2)) / (2 * n)
            e_bar = over_chains(mu, e_mu, 2 * n, (0, 2)) / (2 * n) + U * np.abs(mu_bar)
            d = mu - mu_bar[None, :, None]
            e_d = e_mu + e_bar[None, :, None] + U * np.abs(d)
            SB, eSB = (d * d).sum(axis=(0, 2)), over_chains(d * d, 2.0 * np.abs(d) * e_d + U * d * d, 2 * n, (0, 2))
            q = (SB / (2 * n - 1)) / (SW / (2 * n))
            rhat = np.sqrt((L - 1) / L + q)
            b_rhat = q * (eSB / SB + eSW / np.abs(SW) + 4.0 * U) / (2.0 * rhat) + 8.0 * U * rhat * rhat
        else:
            b_rhat = np.full(rows, np.inf)
    nan_to_inf = lambda b: np.where(np.isnan(b), np.inf, b)            # noqa: E731  (0 / 0: nothing to bound, the values are NaN)
    return dict(mean=b_mean, within=b_within, rhat=nan_to_inf(b_rhat), tau=nan_to_inf(b_tau))


def direct(hist, levels, center=None, wrap=None):
    """The statistics from the whole history [T, rows, n], the plain way: blocks by reshape, numpy's two-pass var(ddof=1)."""
    T, rows, n = hist.shape
    L = T // 2
    V = np.stack([deviations(hist[t], center, wrap) for t in range(T)])                    # [T, rows, n]
    c = np.zeros(rows) if center is None else np.asarray(center, dtype=np.float64)
    mean = c + V.mean(axis=(0, 2))
    if wrap is not None:
        w = np.asarray(wrap, dtype=bool)
        mean[w] = wrap_pi(mean[w])
    s2 = []
    for l in range(levels):
        m, b = T >> l, 1 << l
        blocks = V[:m * b].reshape(m, b, rows, n).mean(axis=1)
        s2.append(blocks.var(axis=0, ddof=1).mean(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.stack([(2.0 ** l) * s2[l] / s2[0] for l in range(levels)])
        if T >= 4:
            halves = V.reshape(2, L, rows, n)
            W = halves.var(axis=1, ddof=1).mean(axis=(0, 2))
            mu = halves.mean(axis=1)                                                        # [2, rows, n]
            BL = np.stack([mu[:, r, :].reshape(-1).var(ddof=1) for r in range(rows)])
            rhat = np.sqrt(((L - 1) / L * W + BL) / W)
        else:
            rhat = np.full(rows, np.nan)
    return dict(mean=mean, within=s2[0], rhat=rhat, tau=tau)


def assert_within(got, want, bounds, what, circular=None):
    """Every statistic of `got` within `bounds` of `want`; NaN exactly where `want` is NaN.  -> the largest error / bound."""
    worst = 0.0
    for k in ("mean", "within", "rhat", "tau"):
        g, w, b = np.asarray(got[k]), np.asarray(want[k]), np.asarray(bounds[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k, g, w)
        diff = np.abs(g - w)
        if k == "mean" and circular is not None:
            diff = np.where(np.asarray(circular, dtype=bool), np.abs(wrap_pi(g - w)), diff)
        ok = ~np.isnan(w)
        assert np.all(diff[ok] <= b[ok]), (what, k, float(np.max(diff[ok] / b[ok])))
        if ok.any() and np.all(b[ok] > 0):
            worst = max(worst, float(np.max(diff[ok] / b[ok])))
    return worst


# ---- fixtures of both files ----------------------------------------------------------------------------------------------------------
def history(T, rows, n, seed=0):
    """A history [T, rows, n] float32 with per-row centres and flags.  Row r by r % 4: 0 a coordinate at 100 m with a spread of
    5 cm; 1 a heading centred at pi - 0.01 whose values straddle the seam (chain 0's first two states are a pair across +-pi);
    2 a constant row (every chain at its centre + 0.5: the sums are exact, within = 0 and R-hat = 0 / 0); 3 a slowly mixing
    coordinate at -20 m (an AR(1) of phi = 0.8, a different level per chain) -> (hist, center [rows], wrap [rows] uint8)."""
    rng = np.random.default_rng(1000 * seed + 17 * T + 3 * rows + n)
    hist, center, wrap = np.zeros((T, rows, n)), np.zeros(rows), np.zeros(rows, dtype=np.uint8)
    for r in range(rows):
        kind = r % 4
        if kind == 0:
            center[r] = 100.0 + r
            hist[:, r] = center[r] + 0.05 * rng.standard_normal((T, n))
        elif kind == 1:
            center[r], wrap[r] = PI - 0.01, 1
            hist[:, r] = wrap_pi(center[r] + 0.05 * rng.standard_normal((T, n)))
            hist[0, r, 0], hist[1, r, 0] = PI - 1e-3, -PI + 1e-3
        elif kind == 2:
            center[r] = 7.0
            hist[:, r] = center[r] + 0.5
        else:
            center[r] = -20.0
            x = rng.standard_normal(n)
            for t in range(T):
                x = 0.8 * x + 0.6 * rng.standard_normal(n)
                hist[t, r] = center[r] + 2.0 * x + (np.arange(n) % 3 - 1) * 0.5
    return hist.astype(np.float32), center, wrap


def level_choices(T):
    return sorted({1, min(2, max_levels(T)), max_levels(T)})


# ---- 0. the names ----------------------------------------------------------------------------------------------------------------------
def test_new_names_are_exported_and_declared():
    assert all(name in nh.EXPORTS for name in NEW)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nfisam_hip.h")).read(), flags=re.S)
    assert all(re.search(r"\b%s\s*\(" % name, hdr) for name in NEW)
    lib = nh.lib()
    assert lib.nfisam_abi_version() == 1600
    assert int(lib.nfisam_chain_state_count(3, 5, 1)) == 4 * 15 and int(lib.nfisam_chain_state_count(3, 5, 4)) == 13 * 15
    assert int(lib.nfisam_chain_state_count(2342, 500, 16)) == 49 * 2342 * 500
    for bad in ((0, 5, 1), (3, 0, 1), (3, 5, 0), (3, 5, 17), (3, 65535 * 64 + 1, 1)):
        assert int(lib.nfisam_chain_state_count(*bad)) == 0, bad
    assert nh.chain_max_levels(2) == 1 and nh.chain_max_levels(14) == 3 and nh.chain_max_levels(64) == 6
    assert nh.chain_max_levels(1 << 20) == 16 and ST.BLOCKING_MIN_DOF == 64 and ST.BLOCKING_PLATEAU == 4.0


# ---- 1. the restatement against the direct form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 4, 6, 14, 64, 200])
@pytest.mark.parametrize("n", [1, 2, 65])
def test_restatement_matches_the_direct_form(T, n):
    hist, center, wrap = history(T, 5, n)
    for levels in sorted({1, max_levels(T)}):
        state, abs_state = record_history(hist, levels, center, wrap)
        got, want = finish(state, T, levels, center, wrap), direct(hist, levels, center, wrap)
        bounds = finish_bounds(state, abs_state, T, levels, center)
        # the constant row: exact sums, no spread
        assert got["within"][2] == 0.0 and np.isnan(got["rhat"][2]) and np.all(np.isnan(got["tau"][:, 2]))
        want["rhat"][2], want["tau"][:, 2] = np.nan, np.nan          # (the direct form's 0 / 0 as well; its within is 0 too)
        assert want["within"][2] == 0.0
        worst = assert_within(got, want, bounds, (T, n, levels), circular=wrap)
        assert np.all(got["tau"][0][[0, 1, 3, 4]] == 1.0)
        # the bound says something: far below the statistics themselves on the rows with spread
        live = [0, 1, 3, 4]
        assert np.all(bounds["within"][live] < 1e-6 * got["within"][live])
        print("T = %d, n = %d, levels = %d: the largest |restatement - direct| / bound = %.3f" % (T, n, levels, worst))


def test_the_cascade_counts_complete_blocks_only():
    """T = 14 leaves values over at every level above 0: level 1 has 7 blocks, level 2 has 3 (of 12 values), and the pending
    slots hold the means of what was left."""
    T, levels = 14, 3
    v = np.arange(1.0, T + 1.0).reshape(T, 1, 1)
    state = np.zeros((slots(levels), 1, 1))
    for t in range(T):
        fold_values(state, v[t], t, T, levels)
    assert state[0, 0, 0] == 28.0 and state[1, 0, 0] == 77.0 and state[2, 0, 0] + state[3, 0, 0] == np.sum(v * v)
    b1, b2 = v.reshape(7, 2).mean(axis=1), v[:12].reshape(3, 4).mean(axis=1)
    assert state[5, 0, 0] == b1.sum() and state[6, 0, 0] == np.sum(b1 * b1)
    assert state[8, 0, 0] == b2.sum() and state[9, 0, 0] == np.sum(b2 * b2)
    assert state[7, 0, 0] == 13.5                                     # the pending level-2 value: the mean of the values 13, 14


# ---- 2. known processes -----------------------------------------------------------------------------------------------------------------------
def ar1(phi, T, n, rng):
    """n stationary AR(1) chains of T values with marginal variance 1 -> [T, 1, n] float32."""
    x = rng.standard_normal(n)
    out = np.empty((T, 1, n))
    for t in range(T):
        x = phi * x + np.sqrt(1.0 - phi * phi) * rng.standard_normal(n)
        out[t, 0] = x
    return out.astype(np.float32)


def block_mean_variance(phi, b):
    """V(b): the variance of the mean of b consecutive values of a unit-variance AR(1)."""
    b = float(b)
    return ((1.0 + phi) / (1.0 - phi) - 2.0 * phi * (1.0 - phi ** b) / (b * (1.0 - phi) ** 2)) / b


def expected_tau(phi, T, levels):
    """2^l E[s2_l] / E[s2_0] with E[s2_l] = m / (m - 1) (V(2^l) - V(m 2^l)), m = T >> l."""
    e = []
    for l in range(levels):
        m = T >> l
        e.append(m / (m - 1.0) * (block_mean_variance(phi, 1 << l) - block_mean_variance(phi, m << l)))
    return np.array([(2.0 ** l) * e[l] / e[0] for l in range(levels)])


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("n,T", [(256, 1000), (130, 200)])
def test_ar1_chains_give_the_expected_blocking_curve(phi, n, T):
    levels = max_levels(T)
    hist = ar1(phi, T, n, np.random.default_rng(20261 + int(100 * phi)))
    state, _ = record_history(hist, levels)
    out = finish(state, T, levels)
    want = expected_tau(phi, T, levels)
    m = T >> np.arange(levels)
    se = want * np.sqrt(2.0 / (n * (m - 1.0)))
    dev = np.abs(out["tau"][:, 0] - want) / se
    print("phi = %.1f, n = %d, T = %d: tau = %s, expected %s, deviation / standard error = %s, R-hat = %.4f"
          % (phi, n, T, np.array2string(out["tau"][:, 0], precision=2), np.array2string(want, precision=2),
             np.array2string(dev, precision=2), out["rhat"][0]))
    assert np.all(dev[1:] <= 5.0) and out["tau"][0, 0] == 1.0
    if T == 1000:                                                     # (at T = 200 and phi = 0.9 a half-chain is 5 tau long:
        assert out["rhat"][0] < 1.05                                  #  R-hat = sqrt(1 + (tau - 1) / L) = 1.08 is the right answer)


def test_shifted_chains_raise_rhat():
    n, T = 64, 64
    hist = ar1(0.0, T, n, np.random.default_rng(7))
    state, _ = record_history(hist, max_levels(T))
    assert finish(state, T, max_levels(T))["rhat"][0] < 1.05
    hist[:, 0, :n // 2] += np.float32(3.0)                            # half the chains three spreads away
    state, _ = record_history(hist, max_levels(T))
    rhat = finish(state, T, max_levels(T))["rhat"][0]
    print("half the chains shifted by 3 spreads: R-hat = %.3f" % rhat)
    assert rhat > 1.5


# ---- 3. circular rows ---------------------------------------------------------------------------------------------------------------------------
def test_a_circular_row_across_the_seam_is_the_same_row_about_zero():
    T, n, levels = 64, 65, 6
    rng = np.random.default_rng(3)
    c = PI - 0.01
    d = 0.05 * rng.standard_normal((T, 1, n))
    X = wrap_pi(c + d).astype(np.float32)                             # what the chains store: both signs near +-pi
    assert (X > 3.0).any() and (X < -3.0).any()
    v = wrap_pi(X.astype(np.float64) - c)                             # the deviations the kernel forms: the nearest image
    assert np.max(np.abs(v - d)) <= np.spacing(np.float32(PI)) and np.max(np.abs(v)) < 0.3
    circ, _ = record_history(X, levels, [c], [1])
    flat, _ = record_history(v, levels, [0.0], None)                  # the same values as a linear row about 0
    assert np.array_equal(circ, flat)
    a, b = finish(circ, T, levels, [c], [1]), finish(flat, T, levels, [0.0], None)
    for k in ("within", "rhat", "tau"):
        assert np.array_equal(a[k], b[k]), k
    assert -PI <= a["mean"][0] < PI and a["mean"][0] == wrap_pi(np.array([c + b["mean"][0]]))[0]
    assert abs(wrap_pi(np.array([a["mean"][0] - c]))[0]) < 5.0 * 0.05 / np.sqrt(T * n) and a["rhat"][0] < 1.05
    # without the flag the same matrix is two clusters 2 pi apart: the flag is what the result rests on
    naive, _ = record_history(X, levels, [c], None)
    assert finish(naive, T, levels, [c], None)["within"][0] > 1.0 > 100.0 * a["within"][0]


# ---- 4. the conventions of blocking_tau ---------------------------------------------------------------------------------------------------------
def test_blocking_tau_conventions():
    # which levels count: n (m_l - 1) >= 64.  T = 64, n = 4: m = 64, 32, 16, ... -> 252, 124, 60: levels 0 and 1
    tl = np.array([1.0, 1.5, 9.0, 9.0, 9.0, 9.0])
    out = ST.blocking_tau(tl, 64, 4)
    assert out["level"] == 1 and out["tau"] == 1.5 and out["ess"] == 4 * 64 / 1.5 and not out["resolved"]   # a block of 2 < 6
    # exactly 64 counts, 63 does not: the last level of T = 64 has m = 2 blocks per chain
    assert ST.blocking_tau(tl, 64, 64)["level"] == 5 and ST.blocking_tau(tl, 64, 63)["level"] == 4
    assert ST.blocking_tau(tl, 64, 64)["tau"] == 9.0
    # the largest estimate among the levels that count, not the last one
    assert ST.blocking_tau(np.array([1.0, 3.0, 2.0]), 64, 64)["tau"] == 3.0
    # resolved iff the longest counted block >= 4 tau: a block of 8 against tau = 2 and just above
    assert ST.blocking_tau(np.array([1.0, 1.5, 1.8, 2.0]), 64, 64)["resolved"]
    assert not ST.blocking_tau(np.array([1.0, 1.5, 1.8, 2.0 + 1e-9]), 64, 64)["resolved"]
    # nothing counts: one chain of 4 values
    none = ST.blocking_tau(np.array([1.0, 1.2]), 4, 1)
    assert none["level"] == -1 and np.isnan(none["tau"]) and np.isnan(none["ess"]) and not none["resolved"]
    # columns: [levels, columns], a NaN column (no spread) stays NaN and unresolved
    cols = ST.blocking_tau(np.array([[1.0, np.nan, 1.0], [1.2, np.nan, 3.0], [1.1, np.nan, 5.0]]), 64, 64)
    assert np.array_equal(cols["tau"], [1.2, np.nan, 5.0], equal_nan=True) and list(cols["resolved"]) == [False, False, False]
    assert cols["ess"][0] == 64 * 64 / 1.2 and np.isnan(cols["ess"][1])
    # phi = 0.9 (tau = 19) at n = 256, T = 1000, from the exact expectations: blocks up to 256 see the plateau, blocks up to 8 do not
    full = ST.blocking_tau(expected_tau(0.9, 1000, 9), 1000, 256)
    assert full["level"] == 8 and full["resolved"] and 17.0 < full["tau"] < 19.0
    short = ST.blocking_tau(expected_tau(0.9, 1000, 4), 1000, 256)
    assert short["level"] == 3 and not short["resolved"] and short["tau"] < 0.4 * 19.0     # a lower bound, and said to be one
    assert "LOWER bound" in ST.blocking_tau.__doc__
    for bad in (dict(T=63), dict(T=0), dict(n=0), dict(T=True)):
        with pytest.raises(ValueError):
            ST.blocking_tau(tl, **dict(dict(T=64, n=4), **bad))
    with pytest.raises(ValueError, match="levels"):
        ST.blocking_tau(np.ones(7), 64, 4)                            # 7 levels need T >= 128
    with pytest.raises(ValueError, match="levels"):
        ST.blocking_tau(np.ones((2, 2, 2)), 64, 4)


# ---- 5. refusals with no device --------------------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_with_no_device():
    good = dict(x_rows=3, n=5, levels=2, T=8, t=0)
    nh.check_chain_args(**good)
    nh.check_chain_args(**dict(good, levels=3, t=7, center=np.zeros(3), wrap=np.array([0, 1, 0])))
    for bad in (dict(T=7), dict(T=0), dict(T=1), dict(T=-2), dict(t=8), dict(t=-1), dict(levels=0), dict(levels=4), dict(levels=True),
                dict(T=1 << 20, levels=17), dict(x_rows=0), dict(n=0), dict(n=65535 * 64 + 1), dict(center=np.zeros(2)),
                dict(center=np.array([0.0, np.nan, 0.0])), dict(wrap=np.zeros(4)), dict(T=8.0), dict(levels=1.5)):
        with pytest.raises(ValueError):
            nh.check_chain_args(**dict(good, **bad))
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.chain_state(3, 5, 2, "cpu")
    with pytest.raises(ValueError):
        nh.chain_state(3, 5, 17, "cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.chain_record_t(torch.zeros(7, 3, 5, dtype=torch.float64), torch.zeros(3, 5), 0, 8, 2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.chain_finish_t(torch.zeros(7, 3, 5, dtype=torch.float64), 3, 5, 2, 8)


def test_record_option_is_checked_with_no_device():
    # the odd-count rule: of 7 post-warm-up states the first is not recorded
    assert ST.check_chain_options(4, 10, 3, {}) == dict(T=6, first=4, levels=2, center=None)
    assert ST.check_chain_options(4, 10, 2, {}) == dict(T=8, first=2, levels=3, center=None)
    assert ST.check_chain_options(4, 1100, 100, dict(levels=None))["levels"] == 8        # min(8, floor(log2 1000) = 9)
    assert ST.check_chain_options(4, 1100, 100, dict(levels=9))["levels"] == 9
    assert ST.check_chain_options(4, 10, 3, None) is None
    opt = ST.check_chain_options(2, 10, 0, dict(center=[1.0, 2.0]))
    assert opt["center"].dtype == np.float64 and list(opt["center"]) == [1.0, 2.0]
    for steps, warmup, rec in ((10, 9, {}), (10, 10, {}), (3, 2, {}), (10, 3, dict(levels=0)), (10, 3, dict(levels=3)),
                               (10, 3, dict(levels=1.0)), (10, 3, dict(levels=True)), (10, 3, dict(depth=2)), (10, 3, True),
                               (10, 3, [2]), (10, 3, dict(center=[0.0] * 3)), (10, 3, dict(center=[0.0, 0.0, np.inf, 0.0]))):
        with pytest.raises(ValueError):
            ST.check_chain_options(4, steps, warmup, rec)
    # diagnostics asks for the 4 states split-R-hat needs: 5 post-warm-up steps record 4, 4 record 4, 3 record 2
    assert ST.check_chain_options(4, 8, 3, {}, least=4)["T"] == 4 and ST.check_chain_options(4, 7, 3, {}, least=4)["T"] == 4
    with pytest.raises(ValueError, match="at least 4 recorded states"):
        ST.check_chain_options(4, 6, 3, {}, least=4)
    # metropolis_refine_t makes the check before it looks for a device: a bad `record` is a ValueError on a CPU tensor, a good
    # one gets as far as the device check
    X, f = torch.zeros(4, 8), (lambda Xt: None)
    with pytest.raises(ValueError, match="recorded states"):
        ST.metropolis_refine_t(X, f, f, 5, 0.1, warmup=4, record={})
    with pytest.raises(ValueError, match="record"):
        ST.metropolis_refine_t(X, f, f, 8, 0.1, warmup=4, record=dict(levels=3))
    with pytest.raises(ValueError, match="record"):
        ST.metropolis_refine(np.zeros((8, 4)), f, f, 8, 0.1, warmup=4, record="yes", device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.metropolis_refine_t(X, f, f, 8, 0.1, warmup=4, record={})


def test_c_entries_refuse_before_any_launch():
    """Every refusal of the two entries returns before a launch, so it can be seen with no device: the pointers are host
    arrays that a launch would never survive, and they keep their bits."""
    lib = nh.lib()
    X, st = np.ones((3, 5), dtype=np.float32), np.zeros(7 * 15)
    out = np.zeros(5 * 3)
    ptr = lambda a: C.c_void_p(a.ctypes.data)                          # noqa: E731
    null = C.c_void_p(0)

    def rec(Xp=ptr(X), sp=ptr(st), rows=3, n=5, levels=2, t=0, T=8):
        return lib.nfisam_chain_record(Xp, sp, rows, n, levels, null, null, C.c_uint32(t), C.c_uint32(T), null)

    def fin(sp=ptr(st), rows=3, n=5, levels=2, T=8, mp=ptr(out), wp=ptr(out[3:]), rp=ptr(out[6:]), tp=ptr(out[9:])):
        return lib.nfisam_chain_finish(sp, rows, n, levels, C.c_uint32(T), null, null, mp, wp, rp, tp, null)

    for bad in (dict(Xp=null), dict(sp=null), dict(rows=0), dict(n=0), dict(n=65535 * 64 + 1), dict(T=7), dict(T=0), dict(T=1),
                dict(t=8), dict(t=9), dict(levels=0), dict(levels=4), dict(levels=17, T=1 << 20), dict(levels=-1)):
        assert rec(**bad) == nh.ERR_ARG, bad
    for bad in (dict(sp=null), dict(mp=null), dict(wp=null), dict(rp=null), dict(tp=null), dict(rows=0), dict(n=0),
                dict(n=65535 * 64 + 1), dict(T=7), dict(T=0), dict(levels=0), dict(levels=4), dict(levels=17, T=1 << 20)):
        assert fin(**bad) == nh.ERR_ARG, bad
    assert not st.any() and not out.any() and np.all(X == 1.0)
