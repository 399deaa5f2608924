"""The float64 oracle of the sample modes (mean-shift ascent and merge as include/nfisam_hip.h states them, in numpy, broadcast as
(starts, n, d)), what it says about the bimodal fixture, and the host logic around the device entry: the bandwidth rule, the
table check and every ValueError that must come before a launch.  The GPU tests import the oracle and the fixtures from here.

The oracle takes a dtype: run in np.longdouble it measures its own float64 rounding (no stop iteration differs on the
fixture, positions agree within 1.2e-14 sigma (asserted: 1.8e-14); on the slow sets within 3.2e-14 scaled units), which is what the device tolerances of tests/test_sample_modes_gpu.py rest on."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, Variable, VariableType
from utils import Statistics as ST

TOL, MERGE = 1e-7, 1e-2
BLOCKS = {"xy": [0, 1], "pose": [0, 1, 2], "heading": [2]}       # columns of data()
CIRC = [False, False, True]


def wrap_pi(t):
    """(t + pi) mod 2 pi - pi with the sign of Python's `%`: [-pi, pi), in the dtype of t."""
    t = np.asarray(t)
    pi = t.dtype.type(np.pi)
    return (t + pi) % (2 * pi) - pi


def data(n, seed):
    """Two hypotheses of a pose: 35 % near (100, -40) heading 3.05 -- a mode across the +-pi seam --, the rest near
    (104, -37) heading -1.2.  -> (x [n, 3] float32, a [n] bool: who belongs to the first)."""
    r = np.random.RandomState(seed)
    a = r.rand(n) < 0.35
    xy_a = r.randn(n, 2) * [0.4, 0.6] + [100, -40]
    xy_b = r.randn(n, 2) * [0.5, 0.3] + [104, -37]
    xy = np.where(a[:, None], xy_a, xy_b)
    h_a = wrap_pi(3.05 + 0.15 * r.randn(n))
    h_b = wrap_pi(-1.2 + 0.2 * r.randn(n))
    return np.column_stack([xy, np.where(a, h_a, h_b)]).astype(np.float32), a


def ring(n, seed):
    """A ring of radius 5 +- 0.2 around (50, -20): the density has a ridge, ascents along it converge slowly."""
    r = np.random.RandomState(seed)
    th = r.uniform(0.0, 2.0 * np.pi, n)
    rad = 5.0 + 0.2 * r.randn(n)
    return np.column_stack([50 + rad * np.cos(th), -20 + rad * np.sin(th)]).astype(np.float32)


def square(n, seed):
    """Uniform on a square of side 10 around (50, -20): shallow bumps, the slowest ascents."""
    r = np.random.RandomState(seed)
    return (r.uniform(-5, 5, (n, 2)) + [50, -20]).astype(np.float32)


def bandwidth(x, cols, circ, weights=None):
    """The default rule of utils.Statistics.sample_modes in numpy float64 -> (scale [d], inv_two_sigma2)."""
    x = np.asarray(x, dtype=np.float64)[:, cols]
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    W = w.sum()
    var, res = np.zeros(len(cols)), np.ones(len(cols))
    for e, c in enumerate(circ):
        if c:
            res[e] = np.hypot((w * np.cos(x[:, e])).sum() / W, (w * np.sin(x[:, e])).sum() / W)
        else:
            m = (w * x[:, e]).sum() / W
            var[e] = (w * (x[:, e] - m) ** 2).sum() / W
    sigma = ST.mode_sigma(ST.effective_sample_size(weights, x.shape[0]), [len(cols)])[0]
    return ST.mode_scale(var, res, circ), 1.0 / (2.0 * sigma * sigma)


def oracle_ascent(x, cols, circ, scale, inv, weights=None, max_iters=500, tol=TOL, dtype=np.float64):
    """-> pos [n, d], dens [n], iters [n] (negative: stopped on max_iters without meeting tol), in `dtype` arithmetic."""
    X = np.asarray(x)[:, cols].astype(dtype)                     # float32 points: exact in either dtype
    n, d = X.shape
    circ = np.asarray(circ, dtype=bool)
    sc, inv, tol2 = np.asarray(scale).astype(dtype), dtype(inv), dtype(tol) * dtype(tol)
    w = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    W = dtype(math.fsum(w.astype(np.float64))) if dtype is np.float64 else w.sum()

    def sums(Y):                                                  # Y [a, d] -> numerators [a, d], denominators [a]
        diff = X[None, :, :] - Y[:, None, :]
        diff[..., circ] = wrap_pi(diff[..., circ])
        u = diff * sc
        k = w[None, :] * np.exp(-inv * (u * u).sum(-1))
        return (k[:, :, None] * diff).sum(1), k.sum(1)

    y, it, dens = X.copy(), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=dtype)
    active = np.arange(n)
    while active.size:
        num, den = sums(y[active])
        dead = den == 0                                           # a zero-weight start out of reach: it stays, density 0
        active, num, den = active[~dead], num[~dead], den[~dead]
        delta = num / den[:, None]
        v = y[active] + delta
        v[:, circ] = wrap_pi(v[:, circ])
        y[active] = v
        it[active] += 1
        s = sc * delta
        met = dtype(2) * inv * (s * s).sum(-1) <= tol2
        capped = ~met & (it[active] >= max_iters)
        for idx in (active[met], active[capped]):
            if idx.size:
                dens[idx] = sums(y[idx])[1] / W
        it[active[capped]] *= -1
        active = active[~(met | capped)]
    return y, dens, it


def oracle_merge(pos, dens, circ, scale, inv, weights=None, merge=MERGE, max_modes=16):
    """-> labels [n], founders (start index of every mode), masses, unlabelled; in the dtype of pos."""
    dtype = pos.dtype.type
    n = pos.shape[0]
    circ, sc = np.asarray(circ, dtype=bool), np.asarray(scale).astype(dtype)
    w = np.ones(n, dtype=dtype) if weights is None else np.asarray(weights).astype(dtype)
    labels, founders, masses = -np.ones(n, dtype=np.int64), [], []
    while len(founders) < max_modes:
        cand = np.flatnonzero((labels < 0) & (dens == dens))
        if not cand.size:
            break
        f = cand[np.argmax(dens[cand])]                           # the first of equal maxima: the lowest index
        diff = pos - pos[f]
        diff[:, circ] = wrap_pi(diff[:, circ])
        u = diff * sc
        member = (labels < 0) & (dtype(2) * dtype(inv) * (u * u).sum(-1) <= dtype(merge) * dtype(merge))
        labels[member] = len(founders)
        founders.append(int(f))
        masses.append(w[member].sum() / w.sum())
    return labels, founders, np.asarray(masses, dtype=np.float64), int((labels < 0).sum())


def oracle_modes(x, cols, circ, scale, inv, weights=None, max_iters=500, tol=TOL, merge=MERGE, max_modes=16, dtype=np.float64):
    pos, dens, it = oracle_ascent(x, cols, circ, scale, inv, weights, max_iters, tol, dtype)
    labels, founders, masses, left = oracle_merge(pos, dens, circ, scale, inv, weights, merge, max_modes)
    return dict(pos=pos, dens=dens, iters=it, labels=labels, founders=founders, masses=masses, unlabelled=left)


_cache = {}


def fixture_modes(n, seed, name, dtype=np.float64):
    """The oracle on one block of data(n, seed) with the default bandwidth: computed once, shared, never modified."""
    key = (n, seed, name, dtype)
    if key not in _cache:
        x, a = data(n, seed)
        cols = BLOCKS[name]
        circ = [CIRC[c] for c in cols]
        scale, inv = bandwidth(x, cols, circ)
        _cache[key] = (x, a, cols, circ, scale, inv, oracle_modes(x, cols, circ, scale, inv, dtype=dtype))
    return _cache[key]


def scaled_gap(p, q, circ, scale):
    """max over starts and columns of |scale_e * wrap_e(p - q)|, in float64."""
    diff = np.asarray(p, dtype=np.longdouble) - np.asarray(q, dtype=np.longdouble)
    c = np.asarray(circ, dtype=bool)
    diff[:, c] = wrap_pi(diff[:, c])
    return float(np.abs(diff * np.asarray(scale, dtype=np.longdouble)).max())


# ---- what the oracle says about the fixture ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, 6, 7])
@pytest.mark.parametrize("n", [65, 200])
def test_the_oracle_finds_both_hypotheses_and_who_belongs_to_which(n, seed):
    for name in BLOCKS:
        x, a, cols, circ, scale, inv, o = fixture_modes(n, seed, name)
        assert len(o["founders"]) == 2 and o["unlabelled"] == 0, (name, o["founders"])
        first = o["labels"][np.flatnonzero(a)[0]]
        assert np.array_equal(o["labels"] == first, a), name
        assert np.all(o["iters"] > 0) and o["iters"].max() <= 29, (name, o["iters"].max())
        if (n, seed) == (200, 5):
            assert sorted(o["masses"].tolist()) == [67 / 200, 133 / 200]
        if name != "xy":                                          # the first hypothesis' heading: across the seam, not near 0
            h = o["pos"][o["founders"][int(first)], -1]
            assert abs(wrap_pi(np.float64(h - 3.05))) < 0.1


def test_float64_and_longdouble_oracles_stop_at_the_same_iteration():
    starts, worst = 0, 0.0
    for n in (65, 200):
        for seed in (5, 6, 7):
            for name in BLOCKS:
                x, a, cols, circ, scale, inv, o = fixture_modes(n, seed, name)
                ol = fixture_modes(n, seed, name, np.longdouble)[-1]
                assert np.array_equal(o["iters"], ol["iters"]), (n, seed, name)
                assert np.array_equal(o["labels"], ol["labels"])    # (the founder need not be: a mode's members end within
                #                                                    rounding of one density, and the largest may change)
                worst = max(worst, scaled_gap(o["pos"], ol["pos"], circ, scale) * math.sqrt(2 * inv))
                starts += n
    print("starts", starts, "largest float64 - longdouble position gap in sigmas", worst)
    assert starts == 2385 and worst <= 1.8e-14


@pytest.mark.parametrize("maker, ulps, slowest, radii", [(ring, 4, 86, (1e-6, 1e-5, 1e-4, 1e-3, 0.1)),
                                                         (square, 16, 165, (1e-5, 1e-4, 1e-3, 0.1))])
def test_slow_ascents_round_alike_and_merge_alike_at_any_radius(maker, ulps, slowest, radii):
    """After 8, 30 and 100 fixed iterations the float64 oracle differs from the longdouble one by 3.4e-15 / 2.1e-15 / 2.5e-15
    scaled units on the ring (S = 15.6, the largest |scale * coordinate|: 2 ulp of S) and by 1.1e-14 / 3.2e-14 / 4.8e-15 on the
    square (S = 19.7: 9 ulp).  Asserted with a margin for another libm's exp: 4 and 16 ulp of S.  (The sets are generated here --
    the ring takes 86 iterations at most and the square 165 -- and the square's gap is ten times the 3e-15 measured on other
    sets of this kind; the device bound 1e-12 (1 + S) = 2.1e-11 is still 650 times the largest figure.)
    The merge does not depend on its radius between 1e-6 and 0.1 sigma on the ring, between 1e-5 and 0.1 on the square: there an
    ascent that contracts by 0.99 per iteration and stops at a shift of tol = 1e-7 sigma is still up to tol * 0.99 / 0.01 =
    1e-5 sigma short of its limit, so two members of one mode can end further apart than 1e-6 -- the ascent, not rounding,
    limits how small a merge radius may be (stated where `merge` is documented)."""
    x = maker(200, 9)
    cols, circ = [0, 1], [False, False]
    scale, inv = bandwidth(x, cols, circ)
    S = float(np.abs(x.astype(np.float64) * scale).max())
    for k in (8, 30, 100):
        p64, _, i64 = oracle_ascent(x, cols, circ, scale, inv, max_iters=k, tol=0.0)
        pld, _, _ = oracle_ascent(x, cols, circ, scale, inv, max_iters=k, tol=0.0, dtype=np.longdouble)
        gap = scaled_gap(p64, pld, circ, scale)
        print(maker.__name__, k, "iterations: float64 - longdouble gap in scaled units", gap, "S", S, "ulp of S", np.spacing(S))
        assert np.all(np.abs(i64) == k) and gap <= ulps * np.spacing(S)
    pos, dens, it = oracle_ascent(x, cols, circ, scale, inv)
    print(maker.__name__, "iterations up to", it.max())
    assert it.min() > 0 and abs(int(it.max()) - slowest) <= 1      # none capped at 500
    ref = oracle_merge(pos, dens, circ, scale, inv, merge=MERGE)
    for radius in radii:
        got = oracle_merge(pos, dens, circ, scale, inv, merge=radius)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], radius


def test_a_zero_weight_start_out_of_reach_stays_and_a_constant_column_is_exact():
    x, _ = data(65, 5)
    x = np.vstack([x, [[1e4, 1e4, 0.0]]]).astype(np.float32)
    x[:, 1] = -37.25
    w = np.ones(66)
    w[-1] = 0.0
    cols, circ = BLOCKS["pose"], [False, False, True]
    scale, inv = bandwidth(x, cols, circ, w)
    assert scale[1] == 0.0
    o = oracle_modes(x, cols, circ, scale, inv, w)
    assert o["iters"][-1] == 0 and o["dens"][-1] == 0.0 and np.array_equal(o["pos"][-1], x[-1].astype(np.float64))
    assert np.all(o["pos"][:, 1] == -37.25)
    assert o["masses"][-1] == 0.0 and abs(o["masses"].sum() - 1.0) < 1e-15


# ---- the host logic of utils.Statistics.sample_modes ----------------------------------------------------------------------------
def test_bandwidth_rule():
    assert ST.effective_sample_size(None, 200) == 200.0
    w = np.array([1.0, 1.0, 2.0, 0.0])
    assert ST.effective_sample_size(w, 4) == 16.0 / 6.0
    assert np.array_equal(ST.mode_sigma(200.0, [1, 2, 3]), 200.0 ** (-1.0 / np.array([5.0, 6.0, 7.0])))
    assert ST.mode_sigma(16.0 / 6.0, [2])[0] == (16.0 / 6.0) ** (-1.0 / 6.0)
    R = 0.8
    s = ST.mode_scale([4.0, 0.0, 123.0, 0.0, 0.0], [np.nan, np.nan, R, 1.0, 0.0], [False, False, True, True, True])
    assert s[0] == 0.5 and s[1] == 0.0                            # a zero spread: scale 0
    assert s[2] == 1.0 / np.sqrt(-2.0 * np.log(R))                # an angle: the circular standard deviation
    assert s[3] == 0.0 and s[4] == 0.0                            # a constant angle; one without direction


@pytest.mark.parametrize("kwargs, match", [
    (dict(blocks=[]), "no blocks"),
    (dict(blocks=[[0, 3]]), "outside"),
    (dict(blocks=[list(range(3)) * 6]), "at most 16"),
    (dict(circular=[True]), "circular"),
    (dict(weights=np.ones(5)), "weights"),
    (dict(weights=-np.ones(20)), "weights"),
    (dict(weights=np.zeros(20)), "weights"),
    (dict(sigma=0.0), "sigma"),
    (dict(sigma=[1.0, 2.0, 3.0]), "sigma"),
    (dict(sigma=np.nan), "sigma"),
    (dict(scale=[1.0, 1.0]), "scale"),
    (dict(scale=[1.0, -1.0, 1.0]), "scale"),
    (dict(tol=-1.0), "tol"),
    (dict(tol=np.nan), "tol"),
    (dict(merge=0.0), "merge"),
    (dict(max_iters=0), "max_iters"),
    (dict(max_modes=0), "max_modes"),
    (dict(max_modes=33), "max_modes"),
])
def test_sample_modes_refuses_before_any_launch(kwargs, match):
    """(No device is needed to get these: on a machine without one they are raised all the same.)"""
    x, _ = data(20, 5)
    args = dict(blocks=[[0, 1], [2]])
    args.update(kwargs)
    with pytest.raises(ValueError, match=match):
        ST.sample_modes(x, **args)


def test_sample_modes_refuses_shapes():
    with pytest.raises(ValueError, match="points, columns"):
        ST.sample_modes(np.zeros(5, dtype=np.float32), [[0]])
    with pytest.raises(ValueError, match="no points"):
        ST.sample_modes(np.zeros((0, 2), dtype=np.float32), [[0]])


def test_check_mode_blocks():
    nh.build()
    t = nh.pack_mmd_blocks([2, 3, 1], [1.0, 0.5, 2.0])
    cols = [0, 1, 0, 1, 2, 2]
    nh.check_mode_blocks(t, cols, 3, scale=np.ones(6), wrap=np.zeros(6, dtype=np.uint8))
    nh.check_mode_blocks(t, cols, 3)
    assert np.array_equal(t["inv_two_sigma2"], [0.5, 2.0, 0.125])

    def bad(field, b, value):
        u = t.copy()
        u[field][b] = value
        return u

    for table, match in ((bad("d", 1, 0), "width"), (bad("d", 1, 17), "width"), (bad("col_off", 2, 6), "leave"),
                         (bad("col_off", 0, -1), "leave"), (bad("col_off", 1, 1), "share"),
                         (bad("inv_two_sigma2", 0, 0.0), "inv_two_sigma2"), (bad("inv_two_sigma2", 2, np.inf), "inv_two_sigma2"),
                         (bad("inv_two_sigma2", 1, np.nan), "inv_two_sigma2"), (t[:0], "blocks"),
                         (t.astype(nh.MOMENT_BLOCK_DTYPE), "MMD_BLOCK_DTYPE")):
        with pytest.raises(ValueError, match=match):
            nh.check_mode_blocks(table, cols, 3)
    with pytest.raises(ValueError, match="row"):
        nh.check_mode_blocks(t, cols, 2)
    with pytest.raises(ValueError, match="row"):
        nh.check_mode_blocks(t, [0, 1, 0, -1, 2, 2], 3)
    with pytest.raises(ValueError, match="scale"):
        nh.check_mode_blocks(t, cols, 3, scale=np.ones(5))
    with pytest.raises(ValueError, match="scale"):
        nh.check_mode_blocks(t, cols, 3, scale=[1, 1, 1, -1, 1, 1])
    with pytest.raises(ValueError, match="scale"):
        nh.check_mode_blocks(t, cols, 3, scale=[1, 1, 1, np.inf, 1, 1])
    with pytest.raises(ValueError, match="wrap"):
        nh.check_mode_blocks(t, cols, 3, wrap=np.zeros(7))
    for kw, match in ((dict(max_iters=0), "max_iters"), (dict(tol=-1e-9), "tol"), (dict(merge=0.0), "merge"),
                      (dict(merge=np.inf), "merge"), (dict(max_modes=0), "max_modes"), (dict(max_modes=33), "max_modes")):
        args = dict(max_iters=10, tol=0.0, merge=0.01, max_modes=32)
        nh.check_mode_args(**args)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            nh.check_mode_args(**args)
    for name in ("nfisam_sample_modes", "nfisam_sample_modes_merge"):
        assert name in nh.EXPORTS and hasattr(nh.lib(), name)


def test_host_side_refusals_of_the_c_entry():
    """The entry refuses bad arguments on the host, before it touches the device, and returns OK for n == 0 without a launch
    (the pointers below are never dereferenced: they are not device memory)."""
    nh.build()
    lib = nh.lib()
    assert lib.nfisam_abi_version() == 1600
    blocks = nh.pack_mmd_blocks([2, 3], [1.0, 0.5])
    fake = C.c_void_p(4096)
    outs = ("pos", "dens", "iters", "labels", "n_modes", "mode_pos", "mode_dens", "mode_mass", "unlabelled")

    def modes(Xt=fake, rows=4, n=5, blk=blocks, blk_dev=fake, nb=2, cols=fake, ne=5, max_iters=10, tol=1e-7, merge=1e-2,
              max_modes=16, **out):
        return lib.nfisam_sample_modes(Xt, rows, n, None if blk is None else blk.ctypes.data_as(C.c_void_p), blk_dev, nb, cols, ne,
                                       None, None, None, max_iters, C.c_double(tol), C.c_double(merge), max_modes,
                                       *[out.get(k, fake) for k in outs], None)
    assert modes(n=0) == nh.OK
    for kw in [dict(Xt=None), dict(blk=None), dict(blk_dev=None), dict(cols=None), dict(n=-1), dict(nb=0), dict(nb=65536),
               dict(ne=0), dict(rows=0), dict(max_iters=0), dict(tol=-1e-9), dict(tol=float("nan")), dict(tol=float("inf")),
               dict(merge=0.0), dict(merge=-1.0), dict(merge=float("nan")), dict(merge=float("inf")), dict(max_modes=0),
               dict(max_modes=33)] + [{k: None} for k in outs]:
        assert modes(**kw) == nh.ERR_ARG, kw
        assert modes(**{**kw, "n": 0}) == (nh.ERR_ARG if "n" not in kw else nh.OK), kw     # (n == 0 excuses nothing)
    for field, value in (("d", 0), ("d", -1), ("d", 17), ("inv_two_sigma2", 0.0), ("inv_two_sigma2", -1.0),
                         ("inv_two_sigma2", np.inf), ("inv_two_sigma2", np.nan)):
        bad = blocks.copy()
        bad[field][1] = value
        assert modes(blk=bad) == nh.ERR_ARG, (field, value)

    def remerge(rows=4, n=5, blk=blocks, blk_dev=fake, nb=2, cols=fake, ne=5, merge=1e-2, max_modes=16, pos=fake, dens=fake, **out):
        return lib.nfisam_sample_modes_merge(rows, n, None if blk is None else blk.ctypes.data_as(C.c_void_p), blk_dev, nb, cols, ne,
                                             None, None, None, C.c_double(merge), max_modes, pos, dens,
                                             *[out.get(k, fake) for k in outs[3:]], None)
    assert remerge(n=0) == nh.OK
    for kw in [dict(blk=None), dict(blk_dev=None), dict(cols=None), dict(pos=None), dict(dens=None), dict(n=-1), dict(nb=0),
               dict(nb=65536), dict(ne=0), dict(rows=0), dict(merge=0.0), dict(merge=float("nan")), dict(merge=float("inf")),
               dict(max_modes=0), dict(max_modes=33)] + [{k: None} for k in outs[3:]]:
        assert remerge(**kw) == nh.ERR_ARG, kw
    bad = blocks.copy()
    bad["d"][0] = 17
    assert remerge(blk=bad) == nh.ERR_ARG
    hdr = open(nh.CSRC + "/../../include/nfisam_hip.h").read()
    assert "int nfisam_sample_modes_merge(" in hdr
    assert "int nfisam_sample_modes(" in hdr and "#define NFISAM_MODES_MAX_MODES  32" in hdr
    assert nh.MODES_MAX_D == 16 and nh.MODES_MAX_MODES == 32


class Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


def test_cpu_tensors_are_refused_and_nothing_is_uploaded(monkeypatch):
    refuse = Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    t = nh.pack_mmd_blocks([2], [1.0])
    X = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_modes(X, t, [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_modes(X.numpy(), t, [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_modes_t(X.t().contiguous(), t, [0, 1])
    with pytest.raises(ValueError, match="row"):
        nh.sample_modes(X.numpy(), t, [0, 3], device="cuda")
    with pytest.raises(ValueError, match="no points"):
        nh.sample_modes(X.numpy()[:0], t, [0, 1], device="cuda")
    with pytest.raises(ValueError, match="max_modes"):
        nh.sample_modes(X.numpy(), t, [0, 1], max_modes=33, device="cuda")
    with pytest.raises(ValueError, match="all zero"):
        nh.sample_modes(X.numpy(), t, [0, 1], weights=np.zeros(5), device="cuda")
    assert refuse.calls == 0


def test_posterior_modes_errors_come_before_any_launch(monkeypatch):
    """The errors of `posterior_summary` (same helper, same order) and those of the mode arguments, on a solver whose graph is
    a pose prior and a range factor over {X0, L1}, eliminated but never trained."""
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_modes is NFiSAM.posterior_modes
    nh.build()
    with pytest.raises(RuntimeError, match="posterior_modes: no factor graph"):
        NFiSAM().posterior_modes()
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    s.add_node(X0)
    s.add_node(L1)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    refuse = Refuse()
    for name in ("sample_moments", "sample_moments_t", "sample_modes", "sample_modes_t", "posterior_walk_raw", "upload",
                 "posterior_log_density", "posterior_log_density_t", "factor_graph_log_density", "factor_graph_log_density_t"):
        monkeypatch.setattr(nh, name, refuse)
    X9 = SE2Variable("X9")
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):
        s.posterior_modes()
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):
        s.posterior_modes(own, weights="importance")
    with pytest.raises(ValueError, match="'importance'"):
        s.posterior_modes(own, weights="uniform")
    with pytest.raises(ValueError, match="posterior_modes: variable X9 is not in the elimination ordering"):
        s.posterior_modes(own, variables=[X0, X9])
    with pytest.raises(ValueError, match="X9 is not in the elimination ordering"):
        s.posterior_modes(own, pairs=[(X0, X9)])
    with pytest.raises(ValueError, match="pair"):
        s.posterior_modes(own, pairs=[(X0, L1, X0)])
    with pytest.raises(ValueError, match="no variable"):
        s.posterior_modes(own, variables=[])
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_modes({X0: own[X0]})
    with pytest.raises(ValueError, match="ragged samples"):
        s.posterior_modes({X0: np.zeros((7, 3)), L1: np.zeros((6, 2))})
    with pytest.raises(ValueError, match="no points"):
        s.posterior_modes({X0: np.zeros((0, 3)), L1: np.zeros((0, 2))})
    for w, match in ((np.ones(6), r"\[n\] = \[7\]"), (-np.ones(7), "non-negative"), (np.zeros(7), "all zero"),
                     (np.array([1, 1, np.nan, 1, 1, 1, 1.0]), "finite")):
        with pytest.raises(ValueError, match=match):
            s.posterior_modes(own, weights=w)
    for kw, match in ((dict(sigma=0.0), "sigma"), (dict(sigma=[1.0, 1.0, 1.0]), "sigma"), (dict(tol=-1.0), "tol"),
                      (dict(merge=0.0), "merge"), (dict(max_iters=0), "max_iters"), (dict(max_modes=33), "max_modes")):
        with pytest.raises(ValueError, match="posterior_modes: .*" + match):
            s.posterior_modes(own, **kw)
    W1, W2 = Variable("W1", 9), Variable("W2", 9)
    s._elimination_ordering = list(s._elimination_ordering) + [W1, W2]
    with pytest.raises(ValueError, match="18 columns wide"):
        s.posterior_modes({**own, W1: np.zeros((7, 9)), W2: np.zeros((7, 9))}, pairs=[(W1, W2)])
    assert refuse.calls == 0
