"""k nearest neighbours, ball counts and the estimators built on them -- what needs no GPU: the float64 numpy oracle (brute-force
distances, stable argsort, counts) against closed forms, the host formulas against scipy, and every refusal.  The GPU tests
(test_sample_knn_gpu.py) import the oracle from here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy.special import digamma, gammaln

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from utils import Statistics as ST

U = 2.0 ** -53


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def wrap_pi(t):
    """theta_to_pipi in float64: (t + pi) mod 2 pi - pi, the remainder taken as C's fmod takes it (exact) and made non-negative."""
    m = np.fmod(t + np.pi, 2.0 * np.pi)
    return np.where(m < 0.0, m + 2.0 * np.pi, m) - np.pi


def oracle_dist(x, y, xcols, ycols, scale=None, wrap=None, norm="max", squared=False):
    """All pair distances [m, n] in float64 between the float32 points x [m, x_cols] and y [n, y_cols] over the entries
    (xcols[e], ycols[e]): u_e = scale_e * wrap_e(x_e - y_e); max_e |u_e| (a NaN u poisons it, as it poisons a sum) or
    sqrt(sum_e u_e^2), the sum in ascending e (`squared`: without the root)."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    acc = np.zeros((x.shape[0], y.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for e, (cx, cy) in enumerate(zip(xcols, ycols)):
            t = x[:, cx].astype(np.float64)[:, None] - y[:, cy].astype(np.float64)[None, :]
            if wrap is not None and wrap[e]:
                t = wrap_pi(t)
            u = t if scale is None else np.float64(scale[e]) * t
            acc = acc + u * u if norm == "l2" else np.maximum(acc, np.abs(u))      # (np.maximum hands a NaN on)
        return np.sqrt(acc) if norm == "l2" and not squared else acc


def oracle_knn(D, k, exclude_self=False):
    """The k smallest of every row of D [m, n] by (distance, j): a stable argsort.  A NaN or infinite distance is no candidate;
    slots without one hold +inf / -1.  -> (dist [k, m], idx [k, m] int32)."""
    D = np.where(np.isfinite(D), D, np.inf)
    if exclude_self:
        assert D.shape[0] == D.shape[1]
        D[np.arange(D.shape[0]), np.arange(D.shape[0])] = np.inf
    m, n = D.shape
    order = np.argsort(D, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(D, order, axis=1)
    idx = np.where(np.isfinite(dist), order, -1)
    if n < k:
        dist = np.concatenate([dist, np.full((m, k - n), np.inf)], axis=1)
        idx = np.concatenate([idx, np.full((m, k - n), -1)], axis=1)
    return dist.T.copy(), idx.T.astype(np.int32)


def oracle_count(D, radius, exclude_self=False):
    """#{ j : D[i, j] < radius[i] } (strict; NaN compares false) -> int32 [m]."""
    with np.errstate(invalid="ignore"):
        inside = D < np.asarray(radius, dtype=np.float64)[:, None]
    if exclude_self:
        inside[np.arange(D.shape[0]), np.arange(D.shape[0])] = False
    return inside.sum(axis=1).astype(np.int32)


def oracle_log_sum(eps):
    """(fsum of log(eps_i) over the positive finite ones, how many)."""
    used = (eps > 0) & np.isfinite(eps)
    return math.fsum(np.log(eps[used]).tolist()), int(used.sum())


def standardising_scale(x, circ=None):
    """What `knn_entropy` takes by default, from numpy: 1 / population std (circular std of an angle)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    circ = np.zeros(x.shape[1], dtype=bool) if circ is None else np.asarray(circ, dtype=bool)
    var = x.var(axis=0)
    res = np.hypot(np.cos(x).mean(axis=0), np.sin(x).mean(axis=0))
    return ST.mode_scale(var, res, circ)


def oracle_entropy(x, cols, k=4, circ=None, scale=None, norm="max"):
    """Kozachenko-Leonenko from the oracle's distances and the host formula -> (H, n_used, zeros)."""
    x = np.asarray(x, dtype=np.float32)
    scale = standardising_scale(x, circ) if scale is None else np.asarray(scale, dtype=np.float64)
    wrap = None if circ is None else np.asarray(circ)[cols]
    dist, _ = oracle_knn(oracle_dist(x, x, cols, cols, scale[cols], wrap, norm), k, exclude_self=True)
    ls, used = oracle_log_sum(dist[k - 1])
    h = ST.entropy_from_log_sum(ls, used, len(cols), k, norm, math.fsum(np.log(scale[cols]).tolist()))
    return float(h[0]), used, int((dist[k - 1] == 0).sum())


def oracle_mutual_information(x, a, b, k=4, circ=None, scale=None):
    """KSG-1 from the oracle's distances and counts and the host formula -> (I, n_a, n_b, eps)."""
    x = np.asarray(x, dtype=np.float32)
    scale = standardising_scale(x, circ) if scale is None else np.asarray(scale, dtype=np.float64)
    flags = np.zeros(x.shape[1], dtype=bool) if circ is None else np.asarray(circ, dtype=bool)
    ab = list(a) + list(b)
    eps = oracle_knn(oracle_dist(x, x, ab, ab, scale[ab], flags[ab]), k, exclude_self=True)[0][k - 1]
    n_a = oracle_count(oracle_dist(x, x, a, a, scale[list(a)], flags[list(a)]), eps, exclude_self=True)
    n_b = oracle_count(oracle_dist(x, x, b, b, scale[list(b)], flags[list(b)]), eps, exclude_self=True)
    return ST.ksg_from_counts(n_a, n_b, k), n_a, n_b, eps


# ---- the fixtures of both files ---------------------------------------------------------------------------------------------------
def gaussian(n, d, seed):
    """n float32 draws of N(0, Sigma) with a random Sigma -> (x, the true entropy 1/2 log det(2 pi e Sigma))."""
    rng = np.random.RandomState(seed)
    A = rng.normal(size=(d, d)) + 1.5 * np.eye(d)
    cov = A @ A.T
    x = rng.multivariate_normal(np.zeros(d), cov, size=n).astype(np.float32)
    return x, 0.5 * np.linalg.slogdet(2.0 * np.pi * np.e * cov)[1]


def ring(n, seed, radius=4.0, noise=0.1):
    """A landmark seen by range only: n points on a ring -> (x, log(2 pi radius) + 1/2 log(2 pi e noise^2), the entropy of
    the product of a uniform angle and a Gaussian radius, right to O((noise / radius)^2))."""
    rng = np.random.RandomState(seed)
    phi, r = rng.uniform(-np.pi, np.pi, n), radius + noise * rng.normal(size=n)
    x = np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1).astype(np.float32)
    return x, math.log(2.0 * math.pi * radius) + 0.5 * math.log(2.0 * math.pi * math.e * noise * noise)


def bivariate(n, rho, seed):
    """-> (x [n, 2] float32 with correlation rho, the true mutual information -1/2 log(1 - rho^2))."""
    rng = np.random.RandomState(seed)
    z = rng.normal(size=(n, 2))
    x = np.stack([z[:, 0], rho * z[:, 0] + math.sqrt(1.0 - rho * rho) * z[:, 1]], axis=1).astype(np.float32)
    return x, -0.5 * math.log(1.0 - rho * rho)


def poses(n, seed, nan_at=None, dup=0):
    """n float32 rows [x, y, heading, a, b]: a two-cluster xy, headings that straddle +-pi, two wide columns; `dup` rows are
    copies of earlier ones (exact ties, eps = 0), `nan_at` gets a NaN x."""
    rng = np.random.RandomState(seed)
    side = rng.rand(n) < 0.4
    xy = np.where(side[:, None], [3.0, -1.0], [-2.0, 2.0]) + 0.3 * rng.normal(size=(n, 2))
    th = wrap_pi(np.pi + 0.4 * rng.normal(size=n))
    ab = rng.normal(size=(n, 2)) * [5.0, 0.05]
    x = np.column_stack([xy, th, ab]).astype(np.float32)
    for t in range(min(dup, n // 2)):
        x[n - 1 - t] = x[t]
    if nan_at is not None and nan_at < n:
        x[nan_at, 0] = np.nan
    return x


# ---- 1. the oracle and the host formulas against closed forms ----------------------------------------------------------------------
# The estimators are consistent, not exact: these bounds are on the ORACLE (and the host formulas), never on the device.
@pytest.mark.parametrize("d, seed, measured", [(1, 11, 0.0329), (2, 12, 0.0304), (3, 13, 0.0484)])
def test_oracle_entropy_of_a_gaussian(d, seed, measured):
    """Kozachenko-Leonenko, n = 2000, k = 4, standardised columns, against 1/2 log det(2 pi e Sigma) of a random Sigma.
    Measured for these seeds: +0.03285 (d = 1), -0.03034 (d = 2), -0.04830 (d = 3) nats; twice that is asserted."""
    x, true = gaussian(2000, d, seed)
    h, used, zeros = oracle_entropy(x, list(range(d)), k=4)
    print("d", d, "H", h, "true", true, "error", h - true)
    assert used == 2000 and zeros == 0
    assert abs(h - true) <= 2.0 * measured


def test_oracle_entropy_of_the_ring():
    """2000 points on a ring of radius 4 m with 0.1 m noise: true 2.3405, measured for this seed 2.2885 (error -0.05205; the
    Gaussian figure from the covariance is 4.918: 2.6 nats of negentropy).  Twice the measured error is asserted."""
    x, true = ring(2000, 21)
    h, used, zeros = oracle_entropy(x, [0, 1], k=4)
    cov = np.cov(x.astype(np.float64).T, bias=True)
    gauss = 0.5 * np.linalg.slogdet(2.0 * np.pi * np.e * cov)[1]
    print("ring H", h, "true", true, "error", h - true, "gauss", gauss)
    assert used == 2000 and zeros == 0
    assert abs(h - true) <= 2.0 * 0.0521
    assert gauss - h > 2.5                                         # the negentropy that the covariance cannot see


@pytest.mark.parametrize("rho, seed, measured", [(0.0, 31, 0.0203), (0.6, 32, 0.0104), (0.9, 33, 0.0506)])
def test_oracle_mutual_information_of_a_bivariate_gaussian(rho, seed, measured):
    """KSG-1, n = 2000, k = 4, against -1/2 log(1 - rho^2).  Measured for these seeds: -0.02028 (rho = 0), +0.01035 (0.6),
    +0.05060 (0.9) nats; twice that is asserted."""
    x, true = bivariate(2000, rho, seed)
    mi = oracle_mutual_information(x, [0], [1], k=4)[0]
    print("rho", rho, "I", mi, "true", true, "error", mi - true)
    assert abs(mi - true) <= 2.0 * measured


def test_oracle_order_ties_empty_slots_and_nan():
    x = np.array([[0.0], [1.0], [1.0], [np.nan], [3.0]], dtype=np.float32)
    D = oracle_dist(x, x, [0], [0])
    dist, idx = oracle_knn(D, 4, exclude_self=True)
    assert np.array_equal(idx[:, 0], [1, 2, 4, -1]) and np.array_equal(dist[:, 0], [1.0, 1.0, 3.0, np.inf])
    assert np.array_equal(idx[:, 1], [2, 0, 4, -1]) and np.array_equal(dist[:, 1], [0.0, 1.0, 2.0, np.inf])     # a tie: the lower j
    assert np.all(idx[:, 3] == -1) and np.all(np.isinf(dist[:, 3]))                                            # a NaN query
    assert np.array_equal(oracle_count(D, [1.0, 1.0, 1.5, 9.0, np.nan], exclude_self=True), [0, 1, 2, 0, 0])     # strict
    assert np.array_equal(oracle_count(D, [-1.0] * 5), [0] * 5) and oracle_count(D, [1e-9] * 5)[1] == 2
    y = np.array([[-3.1], [3.1]], dtype=np.float32)
    assert abs(oracle_dist(y, y, [0], [0], wrap=[1])[0, 1] - (2 * np.pi - 6.2)) < 1e-6


# ---- 2. the host formulas against scipy ----------------------------------------------------------------------------------------------
def _harmonic(j):
    return float(np.sum(1.0 / np.arange(1, max(int(j), 1))))


def _psi_err(j):
    """The error of digamma_table's entry j in units of u: |psi(j)| for the compensated sum's one rounding (and gamma's own),
    H_(j-1) / 2 for the roundings of the terms 1 / i."""
    return abs(float(digamma(j))) + 0.5 * _harmonic(j)


def test_digamma_table():
    t = ST.digamma_table(3000)
    assert np.isnan(t[0]) and t[1] == -ST.EULER_GAMMA and t.shape == (3001,)
    for j in (1, 2, 3, 4, 16, 17, 200, 1999, 2000, 3000):
        assert abs(t[j] - digamma(j)) <= 2.0 * U * _psi_err(j), j      # (twice: scipy's digamma is itself within an ulp)


@pytest.mark.parametrize("norm", ["max", "l2"])
def test_entropy_from_log_sum_against_scipy(norm):
    """H is a sum of five terms.  Their own errors, in units of u times their magnitude: psi(n_used) and psi(k) <= 1.5
    (`_psi_err`), log c_d <= 4 (a log or lgamma of an ulp each, a product, a difference), (d / n_used) log_sum 1 (two
    roundings), the scale term 0 (given); the four additions add u / 2 of a partial sum each, every partial sum at most
    S = sum of the magnitudes.  Together <= (4 + 2) u S; scipy's side of the comparison is built the same way from functions
    good to an ulp: <= 3 u S.  Bound: 9 u S."""
    rng = np.random.RandomState(3)
    for d in (1, 2, 3, 5, 16):
        for k in (1, 4, 16):
            for nu in (17, 200, 2000):
                log_sum, ls = float(rng.normal() * nu), float(rng.normal())
                got = ST.entropy_from_log_sum(log_sum, nu, d, k, norm, ls)[0]
                logc = d * math.log(2.0) if norm == "max" else 0.5 * d * math.log(math.pi) - gammaln(0.5 * d + 1.0)
                terms = [float(digamma(nu)), -float(digamma(k)), float(logc), d / nu * log_sum, -ls]
                assert abs(got - math.fsum(terms)) <= 9.0 * U * sum(abs(t) for t in terms), (d, k, nu)
    both = ST.entropy_from_log_sum([1.0, 2.0], [0, 5], [2, 3], 4)
    assert np.isnan(both[0]) and np.isfinite(both[1]) and both.shape == (2,)
    assert ST.knn_log_unit_ball(2, "l2") == pytest.approx(math.log(math.pi), abs=4 * U) and ST.knn_log_unit_ball(3, "max") == 3 * math.log(2.0)
    with pytest.raises(ValueError, match="norm"):
        ST.knn_log_unit_ball(2, "l1")


def test_ksg_from_counts_against_scipy():
    """I = psi(k) + psi(n) - fsum(2 n table entries) / n.  A table entry j is within u e(j), e(j) = |psi(j)| + H_(j-1) / 2; the
    fsum is exact, so the mean M inherits the mean of the e(j) plus u |M| for its rounding and the division's; the two
    additions add u / 2 of a partial sum each, at most |psi(k)| + |psi(n)| + |M|.  scipy's side: an ulp per digamma, the same
    sums.  Bound: 2 u [e(k) + e(n) + mean e + 2 (|psi(k)| + |psi(n)| + |M|)]."""
    rng = np.random.RandomState(4)
    for n, k in ((1, 1), (17, 4), (200, 1), (2000, 4), (2000, 16)):
        n_a, n_b = rng.randint(0, n, size=n), rng.randint(0, n, size=n)
        got = ST.ksg_from_counts(n_a, n_b, k)
        args = np.concatenate([n_a, n_b]) + 1
        M = math.fsum(digamma(args).tolist()) / n
        ref = float(digamma(k)) + float(digamma(n)) - M
        mean_e = sum(_psi_err(j) for j in args) / n
        bound = 2.0 * U * (_psi_err(k) + _psi_err(n) + mean_e + 2.0 * (abs(digamma(k)) + abs(digamma(n)) + abs(M)))
        assert abs(got - ref) <= bound, (n, k, got - ref, bound)
    assert ST.ksg_from_counts([3, 3, 3, 3], [3, 3, 3, 3], 3) == pytest.approx(digamma(3) - digamma(4), abs=8 * U)
    for bad in (([], []), ([1, 2], [1]), ([1, -1], [1, 1])):
        with pytest.raises(ValueError, match="counts"):
            ST.ksg_from_counts(bad[0], bad[1], 4)


def test_divergence_from_log_sums():
    d = ST.divergence_from_log_sums([10.0, 10.0, 1.0], [4.0, 4.0, 1.0], [50, 49, 50], [50, 50, 50], [2, 2, 3], 50, 70)
    assert d[0] == (2 / 50) * 6.0 + math.log(70 / 49.0) and np.isnan(d[1]) and d[2] == math.log(70 / 49.0)


# ---- 3. every refusal -----------------------------------------------------------------------------------------------------------------
def test_pack_and_check_knn_blocks():
    t = nh.pack_knn_blocks([2, 3, 1], [0, 0, 1])
    assert t.dtype == nh.KNN_BLOCK_DTYPE and t.dtype.itemsize == 16
    assert list(t["col_off"]) == [0, 2, 5] and list(t["d"]) == [2, 3, 1] and list(t["radius_row"]) == [0, 0, 1] and not t["reserved"].any()
    assert not nh.pack_knn_blocks([2, 3])["radius_row"].any()
    cols = [0, 1, 0, 1, 2, 2]
    nh.check_knn_blocks(t, cols, cols, 3, 3, np.ones(6), np.zeros(6, dtype=np.uint8), n_radius=2)
    for mutate, match in [(lambda b: b["d"].__setitem__(1, 0), "width 0 is outside 1..16"),
                          (lambda b: b["d"].__setitem__(1, 17), "width 17 is outside 1..16"),
                          (lambda b: b["col_off"].__setitem__(2, 6), "leave"), (lambda b: b["col_off"].__setitem__(0, -1), "leave"),
                          (lambda b: b["radius_row"].__setitem__(2, 2), "radius_row 2 is out of range"),
                          (lambda b: b["radius_row"].__setitem__(0, -1), "radius_row -1 is out of range")]:
        bad = t.copy()
        mutate(bad)
        with pytest.raises(ValueError, match=match):
            nh.check_knn_blocks(bad, cols, cols, 3, 3, n_radius=2)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_knn_blocks(t, [0, 1, 0, 1, 3, 2], cols, 3, 3)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_knn_blocks(t, cols, [0, 1, 0, -1, 2, 2], 3, 3)
    with pytest.raises(ValueError, match="same length"):
        nh.check_knn_blocks(t, cols, cols[:5], 3, 3)
    with pytest.raises(ValueError, match="scale must have one value per entry"):
        nh.check_knn_blocks(t, cols, cols, 3, 3, scale=np.ones(5))
    with pytest.raises(ValueError, match="scale must be finite"):
        nh.check_knn_blocks(t, cols, cols, 3, 3, scale=[1, 1, np.inf, 1, 1, 1])
    with pytest.raises(ValueError, match="KNN_BLOCK_DTYPE"):
        nh.check_knn_blocks(nh.pack_mmd_blocks([2], [1.0]), [0, 1], [0, 1], 3, 3)
    with pytest.raises(ValueError, match="1..65535 blocks"):
        nh.check_knn_blocks(t[:0], cols, cols, 3, 3)
    assert nh.check_knn_args(5, 7, 4, "max") == 0 and nh.check_knn_args(5, 5, 16, "l2", True) == 1
    for args, match in [((0, 5), "at least one point"), ((5, 0), "at least one point"), ((5, 5, 0), "k must be"),
                        ((5, 5, 17), "k must be"), ((5, 5, 2.5), "k must be"), ((5, 5, 4, "l1"), "norm must be"),
                        ((5, 6, 4, "max", True), "exclude_self"), ((65535 * 64 + 1, 5), "out of range")]:
        with pytest.raises(ValueError, match=match):
            nh.check_knn_args(*args)


def test_host_side_refusals_of_the_c_entries():
    """The entries refuse bad arguments on the host, before they touch the device (the pointers below are never
    dereferenced: they are not device memory)."""
    nh.build()
    lib = nh.lib()
    assert lib.nfisam_abi_version() == 1600
    blocks = nh.pack_knn_blocks([2, 3], [0, 1])
    fake = C.c_void_p(4096)

    def knn(Xt=fake, xr=4, m=5, Yt=fake, yr=4, n=5, ex=0, blk=blocks, blk_dev=fake, nb=2, xc=fake, yc=fake, ne=5, k=4, norm=0,
            dist=fake):
        return lib.nfisam_sample_knn(Xt, xr, m, Yt, yr, n, ex, None if blk is None else blk.ctypes.data_as(C.c_void_p), blk_dev, nb,
                                     xc, yc, ne, None, None, k, norm, dist, None, None, None, None)

    def ball(Xt=fake, xr=4, m=5, Yt=fake, yr=4, n=5, ex=0, blk=blocks, blk_dev=fake, nb=2, xc=fake, yc=fake, ne=5, norm=0,
             radius=fake, nr=2, count=fake):
        return lib.nfisam_sample_ball_count(Xt, xr, m, Yt, yr, n, ex, None if blk is None else blk.ctypes.data_as(C.c_void_p),
                                            blk_dev, nb, xc, yc, ne, None, None, norm, radius, nr, count, None)

    shared = [dict(Xt=None), dict(Yt=None), dict(blk=None), dict(blk_dev=None), dict(xc=None), dict(yc=None), dict(m=0), dict(n=0),
              dict(m=-1), dict(xr=0), dict(yr=0), dict(ne=0), dict(nb=0), dict(nb=65536), dict(m=65535 * 64 + 1),
              dict(n=65535 * 64 + 1), dict(norm=2), dict(norm=-1), dict(ex=1, n=6)]
    for kw in shared + [dict(dist=None), dict(k=0), dict(k=17), dict(k=-1)]:
        assert knn(**kw) == nh.ERR_ARG, kw
    for kw in shared + [dict(radius=None), dict(count=None), dict(nr=0), dict(nr=1)]:    # (nr = 1: block 1 names row 1)
        assert ball(**kw) == nh.ERR_ARG, kw
    for value in (0, -1, 17):
        bad = blocks.copy()
        bad["d"][1] = value
        assert knn(blk=bad) == nh.ERR_ARG and ball(blk=bad) == nh.ERR_ARG, value
    bad = blocks.copy()
    bad["radius_row"][0] = -1
    assert ball(blk=bad) == nh.ERR_ARG
    for name in ("nfisam_sample_knn", "nfisam_sample_ball_count"):
        assert name in nh.EXPORTS and hasattr(lib, name)
    hdr = open(nh.CSRC + "/../../include/nfisam_hip.h").read()
    assert "int nfisam_sample_knn(" in hdr and "int nfisam_sample_ball_count(" in hdr and "} nfisam_knn_block;" in hdr
    for line in ("#define NFISAM_KNN_MAX_D     16", "#define NFISAM_KNN_MAX_K     16", "#define NFISAM_KNN_NORM_MAX  0",
                 "#define NFISAM_KNN_NORM_L2   1"):
        assert line in hdr
    assert nh.KNN_MAX_D == 16 and nh.KNN_MAX_K == 16 and nh.KNN_NORMS == {"max": 0, "l2": 1}
    assert "sample_knn" in open(nh.CSRC + "/Makefile").read() and "sample_knn.hip" in open(nh.CSRC + "/sample_common.h").read()


class Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


def test_cpu_tensors_are_refused_and_nothing_is_uploaded(monkeypatch):
    refuse = Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    t = nh.pack_knn_blocks([2])
    X = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_knn(X, None, t, [0, 1], [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_knn(X.numpy(), None, t, [0, 1], [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_knn_t(X.t().contiguous(), None, t, [0, 1], [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_ball_count(X, None, t, [0, 1], [0, 1], np.ones((1, 5)))
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_ball_count_t(X.t().contiguous(), None, t, [0, 1], [0, 1], torch.ones(1, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="out of range"):
        nh.sample_knn(X.numpy(), None, t, [0, 3], [0, 1], device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        nh.sample_knn(X.numpy(), X.numpy()[:, :1], t, [0, 1], [0, 1], device="cuda")
    with pytest.raises(ValueError, match="k must be"):
        nh.sample_knn(X.numpy(), None, t, [0, 1], [0, 1], k=17, device="cuda")
    with pytest.raises(ValueError, match="exclude_self"):
        nh.sample_knn(X.numpy(), X.numpy()[:4], t, [0, 1], [0, 1], exclude_self=True, device="cuda")
    with pytest.raises(ValueError, match="at least one point"):
        nh.sample_knn(X.numpy()[:0], None, t, [0, 1], [0, 1], device="cuda")
    with pytest.raises(ValueError, match="radius must be"):
        nh.sample_ball_count(X.numpy(), None, t, [0, 1], [0, 1], np.ones((1, 4)), device="cuda")
    with pytest.raises(ValueError, match="radius_row 0 is out of range|radius must be"):
        nh.sample_ball_count(X.numpy(), None, t, [0, 1], [0, 1], np.ones((0, 5)), device="cuda")
    with pytest.raises(ValueError, match="radius_row 1 is out of range"):
        nh.sample_ball_count(X.numpy(), None, nh.pack_knn_blocks([2], [1]), [0, 1], [0, 1], np.ones((1, 5)), device="cuda")
    assert refuse.calls == 0


@pytest.mark.parametrize("call, kwargs, match", [
    ("knn_entropy", dict(k=0), "k must be"), ("knn_entropy", dict(k=17), "k must be"), ("knn_entropy", dict(k=2.5), "k must be"),
    ("knn_entropy", dict(norm="l1"), "norm must be"), ("knn_entropy", dict(k=8), "no 8-th neighbour"),
    ("knn_entropy", dict(scale=[1.0, 1.0]), "scale"), ("knn_entropy", dict(scale=[1.0, -1.0, 1.0]), "scale"),
    ("knn_entropy", dict(scale=[1.0, np.nan, 1.0]), "scale"), ("knn_entropy", dict(blocks=[]), "no blocks"),
    ("knn_entropy", dict(blocks=[[0, 3]]), "outside the 3 columns"), ("knn_entropy", dict(blocks=[list(range(17))]), "at most 16"),
    ("knn_entropy", dict(circular=[True]), "circular"),
    ("knn_mutual_information", dict(norm="l2"), "norm must be 'max'"), ("knn_mutual_information", dict(blocks=[([0], [1], [2])]), "pair 0"),
    ("knn_mutual_information", dict(blocks=[([0], [3])]), "outside"), ("knn_mutual_information", dict(blocks=[]), "no pairs"),
    ("knn_mutual_information", dict(blocks=[([0] * 9, [1] * 8)]), "at most 16"), ("knn_mutual_information", dict(k=8), "neighbour"),
    ("knn_divergence", dict(k=0), "k must be"), ("knn_divergence", dict(blocks=[([0, 1], [0])]), "equal length"),
    ("knn_divergence", dict(blocks=[([0], [2])]), "outside its sample set"), ("knn_divergence", dict(k=7), "at least k"),
    ("knn_divergence", dict(norm="l1"), "norm must be"),
])
def test_the_estimators_refuse_before_any_launch(monkeypatch, call, kwargs, match):
    refuse = Refuse()
    for name in ("upload", "sample_knn_t", "sample_ball_count_t", "sample_moments_t", "_columns"):
        monkeypatch.setattr(nh, name, refuse)
    x, y = np.zeros((8, 3), dtype=np.float32), np.zeros((6, 2), dtype=np.float32)
    kw = dict(kwargs)
    if call == "knn_divergence":
        blocks = kw.pop("blocks", [[0, 1]])
        args = (x, y, blocks)
    elif call == "knn_mutual_information":
        args = (x, kw.pop("blocks", [([0], [1, 2])]))
    else:
        args = (x, kw.pop("blocks", [[0, 1], [2]]))
    with pytest.raises(ValueError, match=match):
        getattr(ST, call)(*args, device="cuda", **kw)
    with pytest.raises(ValueError, match="points, columns"):
        getattr(ST, call)(*((np.zeros(8),) + args[1:]), device="cuda")
    assert refuse.calls == 0
    assert ST.check_knn_options(3, 4, "l2", [1.0, 0.0, 2.0], m=5, n=4).tolist() == [1.0, 0.0, 2.0]
    assert ST.check_knn_options(3, 16, "max", None, m=17) is None


def test_posterior_information_errors_come_before_any_launch(monkeypatch):
    """On a solver whose graph is a pose prior and a range factor over {X0, L1}, eliminated but never trained."""
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_information is NFiSAM.posterior_information
    nh.build()
    with pytest.raises(RuntimeError, match="posterior_information: no factor graph"):
        NFiSAM().posterior_information()
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    s.add_node(X0)
    s.add_node(L1)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    refuse = Refuse()
    for name in ("sample_moments", "sample_moments_t", "sample_knn", "sample_knn_t", "sample_ball_count", "sample_ball_count_t",
                 "posterior_walk_raw", "upload", "_columns"):
        monkeypatch.setattr(nh, name, refuse)
    X9 = SE2Variable("X9")
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):
        s.posterior_information()
    with pytest.raises(ValueError, match="posterior_information: variable X9 is not in the elimination ordering"):
        s.posterior_information(own, variables=[X0, X9])
    with pytest.raises(ValueError, match="X9 is not in the elimination ordering"):
        s.posterior_information(own, pairs=[(X0, X9)])
    with pytest.raises(ValueError, match="pair"):
        s.posterior_information(own, pairs=[(X0, L1, X0)])
    with pytest.raises(ValueError, match="no variable"):
        s.posterior_information(own, variables=[])
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_information({X0: own[X0]})
    with pytest.raises(ValueError, match="posterior_information: k must be"):
        s.posterior_information(own, k=17)
    with pytest.raises(ValueError, match="posterior_information: 7 points have no 7-th neighbour"):
        s.posterior_information(own, k=7)
    with pytest.raises(ValueError, match="no points"):
        s.posterior_information({X0: own[X0][:0], L1: own[L1][:0]})
    with pytest.raises(ValueError, match="the reference holds none"):
        s.posterior_information(own, reference={X9: np.zeros((5, 3))})
    with pytest.raises(ValueError, match=r"reference samples of L1 must be \[m, 2\]"):
        s.posterior_information(own, reference={L1: np.zeros((5, 3))})
    with pytest.raises(ValueError, match="hold no 4-th neighbour"):
        s.posterior_information(own, reference={L1: np.zeros((3, 2))})
    assert refuse.calls == 0
