"""nfisam_sample_density, utils.Statistics.sample_density and posterior_marginal_density on the GPU against the oracles of
test_sample_density_cpu.py: the formula in mpmath at 50 digits for n <= 130, in float64 numpy above that.  No scipy here: its
logpdf comes from tests/golden/sample_density.npz.

THE BOUND is the one derived in the head comment of test_sample_density_cpu.py for ONE float64 evaluation of the formula
(diff exact; the wrap's roundings; |d u_r| <= (r + 1) u sum_c |W_rc diff_c| with absolute values; q; e; the exponent e - M; the
exp's ulps; the sum of non-negative terms; the log's ulps; log W_tot; three final additions), with the DEVICE's figures:
    depth   = ceil(n / 128) * 32 - 1 + 3: a thread adds up to 32 terms of each of the ceil(n / 128) chunks to its running sum,
              then the four waves are added in order (sample_density.hip);
    EXP_ULP, LOG_ULP = the largest error, in ulps of the result, of the device's float64 exp and log against mpmath, MEASURED by
              `device_exp_ulp` and `device_log_ulp` through the entry itself and asserted here to hold:
              exp: one query on one sample, one block per argument a whose log_norm IS a: log_dens = a exactly and
                   dens = exp(a), the device's exp of a known number;
              log: k samples at 0 and one at 1, the query at 0, one block per argument with W = [[w]]: e = (0, .., 0, a) with
                   a = -fl(w^2) / 2, M = 0, and S = fl(k + exp(a)) with the device's exp(a) known from the exp probe; log_norm = 0
                   and log_w = 0 with log_w_sum = 0 make log_dens = log(S), the device's log of a known number in (k, k + 1].
              The constants are the measured values rounded up to one decimal; scripts/sample_density.py --tests records
              them in profiles/density.json.
Against mpmath: |device - exact| <= bound(device).  Against the numpy oracle (n > 130): bound(device) + bound(numpy), the
oracle's own (exp_ulp = log_ulp = 1, depth n).  Against scipy's stored logpdf: the CPU file's bound for that comparison plus
bound(device).  No query is excused anywhere.

The promises are checked as bits: two calls, a block alone / repeated / anywhere in a table of 40, a query at m = 65 and
m = 130 -- and every m in {1, 63, 64, 65} is the first m queries of the m = 130 run whose values were checked."""
import ctypes as C
import json
import math
import os
import random

import mpmath
import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_density_cpu import (POSE_WRAP, U, cloud, fixed_whiten, fixture, log_norm_of, loo_factors, mp_errors, mp_log_density,
                                     oracle_log_density, oracle_loo_scores, population_covariance)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
EXP_ULP = 0.8          # the device's float64 exp against mpmath over [-700, 0] (measured: 0.767): see the head comment
LOG_ULP = 1.4          # the device's float64 log against mpmath over (1, 32] (measured: 1.392)
_worst = {}


def _note(kind, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    live = bound > 0
    ratio = float(np.max(err[live] / bound[live])) if np.any(live) else 0.0
    _worst[kind] = max(_worst.get(kind, 0.0), ratio)
    return ratio


def depth(n):
    return (n + 127) // 128 * 32 - 1 + 3


def _tables(specs):
    """specs: [(qcols, xcols, W [d, d], wrap [d])] -> (blocks, qcols, xcols, wrap), every block its own entries."""
    blocks = nh.pack_density_blocks([len(s[0]) for s in specs], [s[2] for s in specs])
    qc = np.concatenate([np.asarray(s[0]) for s in specs]).astype(np.int32)
    xc = np.concatenate([np.asarray(s[1]) for s in specs]).astype(np.int32)
    wrap = np.concatenate([np.asarray(s[3]) for s in specs]).astype(np.uint8)
    return blocks, qc, xc, wrap


def run(q, x, specs, weights=None, exclude_self=False, want_density=True):
    blocks, qc, xc, wrap = _tables(specs)
    out = nh.sample_density(q, x, blocks, qc, xc, wrap=wrap, weights=weights, exclude_self=exclude_self, want_density=want_density,
                            device=DEV)
    return out["log_density"].cpu().numpy(), None if out["density"] is None else out["density"].cpu().numpy()


def weight_logs(w):
    if w is None:
        return dict()
    with np.errstate(divide="ignore"):
        return dict(log_w=np.log(w), log_w_sum=float(np.log(w.sum())))


def check_block(tag, got, q, x, spec, weights=None, exclude_self=False):
    """One block's device row `got` [m] against the oracle under the bounds of the head comment -> error / bound."""
    qc, xc, W, wrap = spec
    n = x.shape[0]
    kw = dict(weight_logs(weights), exclude_self=exclude_self)
    ref, b_dev = oracle_log_density(q, x, qc, xc, W, wrap, exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(n), **kw)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == -np.inf, ref == -np.inf), tag
    assert not np.any(got == np.inf), tag
    fin = np.isfinite(ref)
    if n <= 130:
        err = mp_errors(got[fin], [v for v, f in zip(mp_log_density(q, x, qc, xc, W, wrap, **kw), fin) if f])
        bound = b_dev[fin]
        kind = "device_vs_mpmath"
    else:
        _, b_np = oracle_log_density(q, x, qc, xc, W, wrap, **kw)
        err, bound, kind = np.abs(got[fin] - ref[fin]), b_dev[fin] + b_np[fin], "device_vs_numpy"
    ratio = _note(kind, err, bound)
    print(tag, kind, "worst error / bound", ratio, "worst |d log|", float(err.max()) if err.size else 0.0)
    assert np.all(err <= bound), (tag, ratio)
    return ratio


def pose_spec(d):
    cols = list(range(d))
    return (cols, cols, fixed_whiten(d), POSE_WRAP[:d])


def queries_for(x, m, seed):
    """m queries: among the samples, some in the tails, one on a sample, one thousands of bandwidths away."""
    q = cloud(m, seed, spread=2.0)
    q[0] = x[0]
    if m > 2:
        q[m - 1, :2] += 4000.0
    return q


# ---- 0. the device's exp and log, measured through the entry ------------------------------------------------------------------------
def _probe_call(x, blocks, log_w, want_density):
    Xt = nh._columns(x, DEV)
    Qt = torch.zeros(1, 1, dtype=torch.float32, device=DEV)
    zero = np.zeros(1, dtype=np.int32)
    return nh.sample_density_t(Qt, Xt, blocks, zero, zero, None, log_w, False, want_density, checked=True, log_w_sum=0.0)


def device_exp(a):
    """The device's exp of every float64 a[b] (finite, <= 0): one sample and one query at 0, block b's log_norm IS a[b]."""
    blocks = nh.pack_density_blocks(np.ones(a.size), [np.eye(1)] * a.size, np.zeros(a.size))
    blocks["log_norm"] = a
    out = _probe_call(np.zeros((1, 1), dtype=np.float32), blocks, None, True)
    assert np.array_equal(out["log_density"].cpu().numpy()[:, 0], a)
    return out["density"].cpu().numpy()[:, 0]


def _ulps(got, exact_of, args):
    worst = 0.0
    with mpmath.workprec(160):
        for g, v in zip(got, args):
            exact = exact_of(mpmath.mpf(float(v)))
            ulp = math.ulp(float(exact)) if float(exact) != 0.0 else 2.0 ** -1074
            worst = max(worst, float(abs(mpmath.mpf(float(g)) - exact) / ulp))
    return worst


def device_exp_ulp(a):
    worst = _ulps(device_exp(a), mpmath.exp, a)
    _worst["device_exp_ulp"] = max(_worst.get("device_exp_ulp", 0.0), worst)
    return worst


def device_log_ulp(w, k):
    """The device's log at S = fl(k + exp(a)), a = -fl(w^2) / 2: k samples at 0 and one at 1, the query at 0, W = [[w]]."""
    a = -0.5 * (w * w)
    S = float(k) + device_exp(a)
    x = np.zeros((k + 1, 1), dtype=np.float32)
    x[k] = 1.0
    blocks = nh.pack_density_blocks(np.ones(w.size), [np.array([[v]]) for v in w], np.zeros(w.size))
    blocks["log_norm"] = 0.0
    got = _probe_call(x, blocks, torch.zeros(k + 1, dtype=torch.float64, device=DEV), False)["log_density"].cpu().numpy()[:, 0]
    worst = _ulps(got, mpmath.log, S)
    _worst["device_log_ulp"] = max(_worst.get("device_log_ulp", 0.0), worst)
    return worst


def test_device_exp_and_log_ulps():
    rng = np.random.RandomState(11)
    a = -np.concatenate([10.0 ** rng.uniform(-3.0, np.log10(700.0), 3000), rng.uniform(0.0, 40.0, 3000), [0.0, 0.5, 1.0, 700.0]])
    worst_exp = device_exp_ulp(a)
    print("device exp: largest error", worst_exp, "ulp over", a.size, "arguments in [-700, 0]")
    w = np.concatenate([rng.uniform(0.01, 6.0, 1500), 10.0 ** rng.uniform(-3.0, 0.0, 500)])
    worst_log = 0.0
    for k in (1, 2, 5, 17, 31):
        worst = device_log_ulp(w, k)
        print("device log: largest error", worst, "ulp over", w.size, "arguments in (%d, %d]" % (k, k + 1))
        worst_log = max(worst_log, worst)
    assert worst_exp <= EXP_ULP and worst_log <= LOG_ULP, (worst_exp, worst_log)


# ---- 1. values where the launch form can go wrong -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 6])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 130, 300])
def test_values_at_every_shape(n, d):
    """m = 130 queries against n samples, every query checked; then m in {1, 63, 64, 65}: the first m of those queries give
    the first m of those results, bit for bit (one lane, and the 64-query tile's edge).  Weighted (one weight zero): 65 queries."""
    x = cloud(n, 100 + n)
    q = queries_for(x, 130, 300 + n)
    spec = pose_spec(d)
    ld, dens = run(q, x, [spec])
    assert ld.shape == (1, 130) and dens.shape == (1, 130)
    check_block("n %d d %d" % (n, d), ld[0], q, x, spec)
    with np.errstate(over="ignore"):
        # dens = exp(log_dens): the device's exp against numpy's (an ulp each; 1e-300 where the result is subnormal)
        assert np.all(np.abs(dens[0] - np.exp(ld[0])) <= 2.0 * U * (EXP_ULP + 1.0) * np.exp(ld[0]) + 1e-300)
    assert np.isfinite(ld[0, 129]) and ld[0, 129] < -1e6 and dens[0, 129] == 0.0
    for m in (1, 63, 64, 65):
        part, pd = run(q[:m], x, [spec])
        assert np.array_equal(part[0], ld[0, :m]) and np.array_equal(pd[0], dens[0, :m]), m
    nod, none = run(q[:65], x, [spec], want_density=False)
    assert none is None and np.array_equal(nod[0], ld[0, :65])
    w = np.random.RandomState(n).uniform(0.1, 2.0, n)
    if n > 2:
        w[1] = 0.0
    lw, _ = run(q[:65], x, [spec], weights=w)
    check_block("n %d d %d weighted" % (n, d), lw[0], q[:65], x, spec, weights=w)


# ---- 2. the promises ----------------------------------------------------------------------------------------------------------------
def test_a_table_of_forty_blocks():
    """40 blocks of widths 1, 2, 3, 6 over overlapping entries; the pose block stands at 0, 17 and 39 (and its xy and heading
    parts elsewhere): its rows equal, bit for bit, the block alone and a second call; a query's bits are those at m = 65."""
    x, q = cloud(200, 7), queries_for(cloud(200, 7), 130, 8)
    Xt, Qt = nh._columns(x, DEV), nh._columns(q, DEV)
    kinds = [pose_spec(3), pose_spec(1), pose_spec(2), pose_spec(6), ([2], [2], fixed_whiten(1, 9) * 3.0, [1]),
             ([3, 4, 5], [3, 4, 5], fixed_whiten(3, 5), [0, 0, 1])]
    order = [0] + [1 + (k % 5) for k in range(16)] + [0] + [1 + ((3 * k) % 5) for k in range(21)] + [0]
    assert len(order) == 40 and order[0] == order[17] == order[39] == 0
    # one entry list, shared: the six columns; a block's col_off is its first column (blocks overlap and repeat entries)
    cols = np.arange(6, dtype=np.int32)
    table = nh.pack_density_blocks([len(kinds[k][0]) for k in order], [kinds[k][2] for k in order], [kinds[k][0][0] for k in order])
    nh.check_density_blocks(table, cols, cols, 6, 6, POSE_WRAP)
    first = nh.sample_density_t(Qt, Xt, table, cols, cols, POSE_WRAP, want_density=True)
    again = nh.sample_density_t(Qt, Xt, table, cols, cols, POSE_WRAP, want_density=True)
    for key in ("log_density", "density"):
        assert torch.equal(first[key], again[key]), key
    alone = {}
    for k, kind in enumerate(kinds):
        t1 = nh.pack_density_blocks([len(kind[0])], [kind[2]], [kind[0][0]])
        alone[k] = nh.sample_density_t(Qt, Xt, t1, cols, cols, POSE_WRAP, want_density=True)
    for at, k in enumerate(order):
        for key in ("log_density", "density"):
            assert torch.equal(first[key][at], alone[k][key][0]), (key, at, k)
    ld = first["log_density"].cpu().numpy()
    for k in (0, 3, 4, 5):                                           # and the values are the oracle's
        check_block("table kind %d" % k, ld[order.index(k)], q, x, kinds[k])
    half = nh.sample_density_t(Qt[:, :65].contiguous(), Xt, table, cols, cols, POSE_WRAP, want_density=True)
    for key in ("log_density", "density"):
        assert torch.equal(half[key], first[key][:, :65]), key
    # wrap None is no wrap: the same bits as flags that are all zero
    plain = nh.sample_density_t(Qt, Xt, table[1:2].copy(), cols, cols, None)
    zeros = nh.sample_density_t(Qt, Xt, table[1:2].copy(), cols, cols, np.zeros(6, dtype=np.uint8))
    assert torch.equal(plain["log_density"], zeros["log_density"])


# ---- 3. scipy's stored logpdf ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("rule", ["scott", "silverman"])
def test_fixture_cases_against_scipy(k, rule):
    fx = fixture()
    x, q = fx["x%d" % k], fx["q%d" % k]
    w = fx["w%d" % k] if "w%d" % k in fx else None
    n, d = x.shape
    cols = list(range(d))
    res = ST.sample_density(x, q, [cols], weights=w, bandwidth=rule, device=DEV)
    got = res["log_density"].cpu().numpy()[0]
    ref = fx["logpdf_%s%d" % (rule, k)]
    cond = float(np.linalg.cond(fx["cov_%s%d" % (rule, k)]))
    # H comes from the device's moments: a two-pass covariance of n terms, (n + 16) u relative to the sum of magnitudes, times
    # the condition number for an entry that cancels (the CPU file's rule for scipy's covariance, with the sum's depth)
    tol_h = (n + 16) * U * cond
    assert np.all(np.abs(res["H"][0] - fx["cov_%s%d" % (rule, k)]) <= tol_h * np.abs(fx["cov_%s%d" % (rule, k)]))
    W = ST.density_whiten(res["H"][0])                               # the device ran with this W: the bound is taken at it
    kw = weight_logs(w)
    _, b = oracle_log_density(q, x, cols, cols, W, None, **kw)
    _, b_scipy = oracle_log_density(q, x, cols, cols, W, None, whitened_points=True, **kw)
    _, b_dev = oracle_log_density(q, x, cols, cols, W, None, exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(n), **kw)
    # the device's H differs from scipy's by (n + 16) u in norm: the quadratic form moves by cond(H) times that, relatively, and
    # log det by d times it: |d log| <= (n + 16) u cond (|log| + d)
    dH = tol_h * (np.abs(ref) + d)
    err = np.abs(got - ref)
    ratio = _note("device_vs_scipy", err, (b + b_scipy) * cond + b_dev + dH)
    print("case", k, rule, "device against scipy: worst |d log|", err.max(), "where the log is", ref[np.argmax(err)], "error / bound", ratio)
    assert np.all(err <= (b + b_scipy) * cond + b_dev + dH)
    check_block("fixture %d %s" % (k, rule), got, q, x, (cols, cols, W, np.zeros(d, dtype=np.uint8)), weights=w)


# ---- 4. semantics ----------------------------------------------------------------------------------------------------------------------
def test_the_heading_seam():
    s = np.array([[np.pi - 0.01], [-(np.pi - 0.01)]], dtype=np.float32)
    p = np.array([[np.pi - 0.005], [-np.pi + 0.002], [0.0]], dtype=np.float32)
    W = np.array([[1.0 / 0.05]])
    ld, _ = run(p, s, [([0], [0], W, [1]), ([0], [0], W, [0])])
    check_block("seam wrapped", ld[0], p, s, ([0], [0], W, [1]))
    check_block("seam plain", ld[1], p, s, ([0], [0], W, [0]))
    assert np.all(ld[0, :2] > ld[1, :2] + 0.3) and abs(ld[0, 0] - ld[0, 1]) < 0.1


@pytest.mark.parametrize("n", [1, 2, 65, 130, 200])
def test_exclude_self(n):
    x = cloud(n, 40 + n)
    specs = [pose_spec(3), pose_spec(1)]
    w = np.random.RandomState(n).uniform(0.1, 2.0, n)
    for weights in (None, w):
        ld, dens = run(x, None, specs, weights=weights, exclude_self=True)
        if n == 1:
            assert np.all(ld == -np.inf) and np.all(dens == 0.0)
            continue
        for b, spec in enumerate(specs):
            check_block("loo n %d block %d %s" % (n, b, "weighted" if weights is not None else "plain"), ld[b], x, x, spec,
                        weights=weights, exclude_self=True)
        with_self, _ = run(x, None, specs, weights=weights)
        assert np.all(with_self != ld)


def test_a_zero_weight_is_a_deleted_point():
    x, q = cloud(150, 3), queries_for(cloud(150, 3), 70, 4)
    spec = pose_spec(3)
    w = np.random.RandomState(1).uniform(0.1, 2.0, 150)
    w[[0, 77, 149]] = 0.0
    keep = w > 0
    full, _ = run(q, x, [spec], weights=w)
    less, _ = run(q, x[keep], [spec], weights=w[keep])
    kw = dict(exp_ulp=EXP_ULP, log_ulp=LOG_ULP)
    _, b1 = oracle_log_density(q, x, *spec, depth=depth(150), **weight_logs(w), **kw)
    _, b2 = oracle_log_density(q, x[keep], *spec, depth=depth(147), **weight_logs(w[keep]), **kw)
    ratio = _note("zero_weight", np.abs(full[0] - less[0]), b1 + b2)
    print("zero weight against deletion: error / bound", ratio)
    assert np.all(np.abs(full[0] - less[0]) <= b1 + b2)
    zero, dz = run(q[:3], x[:2], [spec], weights=np.array([0.0, 1.0]))          # the only weighted sample is the far one, or ..
    assert np.all(np.isfinite(zero))
    lw = torch.full((2,), -np.inf, dtype=torch.float64, device=DEV)               # .. no sample contributes at all
    t = _tables([spec])
    dead = nh.sample_density_t(nh._columns(q[:3], DEV), nh._columns(x[:2], DEV), t[0], t[1], t[2], t[3], lw, want_density=True,
                               checked=True, log_w_sum=0.0)
    assert bool((dead["log_density"] == -np.inf).all()) and bool((dead["density"] == 0.0).all())


def test_nan_queries_and_far_queries():
    x = cloud(140, 5)
    q = queries_for(x, 70, 6)
    q[3, 1] = np.nan
    q[9, 2] = np.nan
    specs = [pose_spec(3), pose_spec(1), ([2], [2], fixed_whiten(1), [1])]
    ld, dens = run(q, x, specs)
    assert np.isnan(ld[0, [3, 9]]).all() and np.isnan(dens[0, [3, 9]]).all()
    assert np.isfinite(ld[1, 3]) and np.isfinite(ld[1, 9]) and np.isnan(ld[2, 9]) and np.isfinite(ld[2, 3])
    assert np.isnan(ld).sum() == 3
    # 1e4 bandwidths from every sample: W = 1 / h with h = 0.01 and a query 100 m beyond the samples
    far = np.array([[float(x[:, 0].max()) + 100.0]], dtype=np.float32)
    fl, fd = run(far, x, [([0], [0], np.array([[100.0]]), [0])])
    print("a query 1e4 bandwidths away: log density", fl[0, 0], "density", fd[0, 0])
    assert np.isfinite(fl[0, 0]) and -1e8 < fl[0, 0] < -4e7 and fd[0, 0] == 0.0
    check_block("far", fl[0], far, x, ([0], [0], np.array([[100.0]]), [0]))


def _raw(Qt, Xt, blocks, blocks_dev, qc, xc, ne, out, dens, q_rows=6, x_rows=6, nb=None, m=None, n=None, ex=0, log_w=None, lws=0.0):
    rc = nh.lib().nfisam_sample_density(C.c_void_p(Qt.data_ptr()), q_rows, int(Qt.shape[1]) if m is None else m, C.c_void_p(Xt.data_ptr()),
                                        x_rows, int(Xt.shape[1]) if n is None else n, ex, blocks.ctypes.data_as(C.c_void_p),
                                        C.c_void_p(blocks_dev.data_ptr()), int(blocks.shape[0]) if nb is None else nb,
                                        C.c_void_p(qc.data_ptr()), C.c_void_p(xc.data_ptr()), ne, None,
                                        None if log_w is None else C.c_void_p(log_w.data_ptr()), C.c_double(lws),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(dens.data_ptr()), None)
    torch.cuda.synchronize()
    return rc


def test_a_bad_block_of_the_device_table_yields_nan_and_leaves_the_others_alone():
    """The host copy is good and passes the entry; the device copy (what the kernel reads) has a row past its matrix, a
    negative row, entries that leave the lists, a width out of range.  Such a block is never walked: its rows are NaN, every
    other block's bits are untouched and nothing is read out of bounds."""
    x, q = cloud(100, 7), queries_for(cloud(100, 7), 70, 8)
    Xt, Qt = nh._columns(x, DEV), nh._columns(q, DEV)
    specs = [pose_spec(3), pose_spec(2), ([3, 4, 5], [3, 4, 5], fixed_whiten(3, 5), [0, 0, 0])]
    blocks, qc, xc, _ = _tables(specs)
    ne = int(qc.size)
    good = nh.sample_density_t(Qt, Xt, blocks, qc, xc, None, want_density=True)

    def check(table, cq, cx, bad_block):
        dev_blocks = nh.upload(table.view(np.uint8).reshape(-1), device=DEV)[0]
        tabs = nh.upload(np.asarray(cq, dtype=np.int32), np.asarray(cx, dtype=np.int32), device=DEV)
        out = torch.full((3, 70), -7.0, dtype=torch.float64, device=DEV)
        dens = torch.full((3, 70), -7.0, dtype=torch.float64, device=DEV)
        assert _raw(Qt, Xt, blocks, dev_blocks, tabs[0], tabs[1], ne, out, dens) == nh.OK
        for b in range(3):
            if b == bad_block:
                assert bool(torch.isnan(out[b]).all()) and bool(torch.isnan(dens[b]).all()), b
            else:
                assert torch.equal(out[b], good["log_density"][b]) and torch.equal(dens[b], good["density"][b]), b

    for which in ("q", "x"):
        for bad_row in (6, -1, 2 ** 30):
            cq, cx = qc.copy(), xc.copy()
            (cq if which == "q" else cx)[4] = bad_row               # entry 4 = the second column of block 1 (entries 3..4)
            check(blocks, cq, cx, 1)
            with pytest.raises(ValueError, match="out of range"):    # the binding's own check refuses it
                nh.sample_density_t(Qt, Xt, blocks, cq, cx, None)
    for off in (ne, -1, ne - 2, 2 ** 31 - 2):                        # past the lists, before them, running out of them from inside
        past = blocks.copy()
        past["col_off"][2] = off
        check(past, qc, xc, 2)
        with pytest.raises(ValueError, match="leave"):
            nh.sample_density_t(Qt, Xt, past, qc, xc, None)
    for width in (0, 7, -3, 2 ** 31 - 1):
        wide = blocks.copy()
        wide["d"][0] = width
        check(wide, qc, xc, 0)
    check(blocks, qc, xc, None)


def test_what_the_entry_refuses_writes_nothing():
    x = cloud(64, 7)
    Xt = nh._columns(x, DEV)
    specs = [pose_spec(3), pose_spec(2)]
    blocks, qc, xc, _ = _tables(specs)
    dev_blocks = nh.upload(blocks.view(np.uint8).reshape(-1), device=DEV)[0]
    tabs = nh.upload(qc, xc, device=DEV)
    lw = torch.zeros(64, dtype=torch.float64, device=DEV)

    def refused(table=blocks, **kw):
        out = torch.full((2, 64), -7.0, dtype=torch.float64, device=DEV)
        dens = torch.full((2, 64), -7.0, dtype=torch.float64, device=DEV)
        assert _raw(Xt, Xt, table, dev_blocks, tabs[0], tabs[1], int(qc.size), out, dens, **kw) == nh.ERR_ARG, kw
        assert bool((out == -7.0).all()) and bool((dens == -7.0).all())

    for kw in (dict(m=0), dict(n=0), dict(q_rows=0), dict(x_rows=0), dict(nb=0), dict(nb=65536), dict(m=65535 * 64 + 1),
               dict(ex=1, m=63), dict(log_w=lw, lws=float("nan")), dict(log_w=lw, lws=float("-inf"))):
        refused(**kw)
    for field, at, value in (("d", None, 0), ("d", None, 7), ("log_norm", None, np.nan), ("whiten", 0, 0.0), ("whiten", 2, -1.0),
                             ("whiten", 1, np.inf)):
        bad = blocks.copy()
        if at is None:
            bad[field][1] = value
        else:
            bad[field][1, at] = value
        refused(bad)
    with pytest.raises(ValueError, match="nfisam_sample_density"):   # and through the binding, past its own checks
        bad = blocks.copy()
        bad["d"][1] = 7
        nh.sample_density_t(Xt, None, bad, qc, xc, None, checked=True)
    out = torch.full((2, 64), -7.0, dtype=torch.float64, device=DEV)  # the same call with good arguments writes all of it
    dens = torch.full((2, 64), -7.0, dtype=torch.float64, device=DEV)
    assert _raw(Xt, Xt, blocks, dev_blocks, tabs[0], tabs[1], int(qc.size), out, dens, ex=1, log_w=lw, lws=float(np.log(64.0))) == nh.OK
    assert not bool((out == -7.0).any()) and not bool((dens == -7.0).any())
    got = out.cpu().numpy()                                           # (unit weights as log_w = 0, no wrap flags: the oracle's)
    for b, spec in enumerate(specs):
        check_block("raw call block %d" % b, got[b], x, x, (spec[0], spec[1], spec[2], np.zeros(len(spec[0]))), weights=np.ones(64),
                    exclude_self=True)


# ---- 5. utils.Statistics: bandwidths from the device's moments, the leave-one-out selection, hpd_level ---------------------------
def test_statistics_sample_density_and_hpd_level():
    x = cloud(300, 21)
    circ = POSE_WRAP.astype(bool)
    q = queries_for(x, 40, 22)
    blocks = [[0, 1], [0, 1, 2], [2], ([3, 4, 5], [0, 1, 2])]
    for given, qq in ((x, q), (torch.from_numpy(x).to(DEV), torch.from_numpy(q).to(DEV))):
        res = ST.sample_density(given, qq, blocks, circular=circ, bandwidth="silverman", want_density=True, device=DEV)
        assert set(res) == {"log_density", "density", "factor", "H", "n_eff"} and res["n_eff"] == 300.0
        ld = res["log_density"].cpu().numpy()
        assert ld.shape == (4, 40) and res["density"].shape == (4, 40)
        for b, blk in enumerate(blocks):
            xc, qc = (blk[0], blk[1]) if isinstance(blk, tuple) else (blk, blk)
            d = len(xc)
            assert res["factor"][b] == ST.density_factor(300.0, d, "silverman")
            mom = nh.sample_moments(x, nh.pack_moment_blocks([d]), xc, circular=POSE_WRAP[xc], device=DEV)[2].cpu().numpy().reshape(d, d)
            assert np.array_equal(res["H"][b], ST.density_bandwidth(mom, 300.0, d, "silverman", circ[xc]))
            check_block("statistics block %d" % b, ld[b], q, x, (qc, xc, ST.density_whiten(res["H"][b]), POSE_WRAP[xc]))
    w = np.random.RandomState(2).uniform(0.0, 2.0, 300)
    res = ST.sample_density(x, None, [[0, 1, 2]], circular=circ, weights=w, bandwidth=0.4)
    own = res["log_density"][0]
    assert res["factor"][0] == 0.4 and abs(res["n_eff"] - w.sum() ** 2 / (w * w).sum()) <= 1e-12 * 300
    at = ST.sample_density(x, q, [[0, 1, 2]], circular=circ, weights=w, bandwidth=0.4)["log_density"][0]
    level = ST.hpd_level(own, at, torch.from_numpy(w).to(DEV))
    assert torch.is_tensor(level) and level.is_cuda
    ref = ST.hpd_level(own.cpu().numpy(), at.cpu().numpy(), w)
    # (two sums of 300 non-negative terms each, in torch's order and in numpy's: (n + 2) u relative apiece)
    assert np.all(np.abs(level.cpu().numpy() - ref) <= 2 * (300 + 2) * U) and ref[0] < 1.0 and ref[39] == 1.0
    with pytest.raises(ValueError, match="no spread"):
        ST.sample_density(np.column_stack([x[:, 0], np.ones(300, dtype=np.float32)]), None, [[0, 1]], device=DEV)


def test_leave_one_out_selection_on_the_bimodal_set():
    x = fixture()["bimodal"].reshape(-1, 1)
    res = ST.sample_density(x, None, [[0]], bandwidth="loo", device=DEV)
    factors = loo_factors(500.0)
    scores, bounds = oracle_loo_scores(x, factors)
    loo = res["loo"][0]
    assert np.array_equal(loo["factors"], factors)
    # the device's scores: the mean of 500 log densities, each within the device's bound of the oracle's (plus the oracle's
    # own bound), the mean by torch within (n + 2) u of the mean of the magnitudes
    cov = nh.sample_moments(x, nh.pack_moment_blocks([1]), [0], device=DEV)[2].cpu().numpy().reshape(1, 1)
    for c, f in enumerate(factors):
        W = ST.density_whiten(ST.density_bandwidth(cov, 500.0, 1, float(f)))
        v, b_dev = oracle_log_density(x, x, [0], [0], W, None, exclude_self=True, exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(500))
        _, b_np = oracle_log_density(x, x, [0], [0], W, None, exclude_self=True)
        bound = float(np.mean(b_dev + b_np) + (500 + 2) * U * np.mean(np.abs(v)))
        ratio = _note("loo_score", abs(loo["scores"][c] - float(np.mean(v))), bound)
        assert abs(loo["scores"][c] - float(np.mean(v))) <= bound, (c, ratio)
    best = int(np.argmax(scores))
    print("leave-one-out: device picks", res["factor"][0], "oracle", factors[best], "scores", loo["scores"])
    assert res["factor"][0] == factors[best] and int(np.argmax(loo["scores"])) == best and ST.DENSITY_LOO_POWERS[best] == -8
    assert abs(np.sqrt(res["H"][0][0, 0]) - 0.09) < 0.005
    wide = ST.sample_density(x, None, [[0]], bandwidth="scott", device=DEV)
    assert np.sqrt(wide["H"][0][0, 0]) > 10 * np.sqrt(res["H"][0][0, 0])


# ---- 6. the solver -----------------------------------------------------------------------------------------------------------------------
def gaussian_tail(z):
    return math.erfc(z / math.sqrt(2.0))


def test_posterior_marginal_density_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem (the fixture and seeds of test_posterior_modes_on_the_small_range_problem).
    A curve's trapezoid integral: the KDE is a mixture of n Gaussians of width h; the grid spans min - 3 h .. max + 3 h, so
    every component keeps at least Phi(3) of its mass on each side: the mass left out is at most Q(z_lo) + Q(z_hi) = 0.0027,
    z the distance from the extreme sample to the grid's end in bandwidths (3, up to the grid's rounding to float32).  The trapezoid rule on a Gaussian mixture of width
    h with step s is off by at most s^2 / 12 max|f''| (max - min + 6 h) <= s^2 / 12 * 0.4 / h^3 * span: evaluated per curve."""
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
    fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
    kwargs = json.loads(str(fx["arguments"]))
    kwargs["cuda_training"] = True
    kwargs["flow_iterations"] = 200
    path = tmp_path / "factor_graph.fg"
    path.write_text(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    nodes, truth, factors = graph_file_parser(str(path), "fg", prior_cov_scale=0.1)
    steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))[:2]
    solver = NFiSAM(NFiSAMArgs(**kwargs))
    for vs, fs in steps:
        for v in vs: solver.add_node(v)
        for f in fs: solver.add_factor(f)
        solver.update_physical_and_working_graphs()
        solver.incremental_inference()
    order = list(solver.elimination_ordering)
    n, g = 200, 400
    pair = (order[0], order[-1])
    assert pair[0].dim + pair[1].dim <= 6

    torch.manual_seed(17)
    drawn = solver.posterior_collect(solver.posterior_launch(n))
    host = np.hstack([np.asarray(drawn[v], dtype=np.float32) for v in order])
    cols, circ, at = {}, [], 0
    for v in order:
        cols[v] = list(range(at, at + v.dim))
        circ.extend(bool(c) for c in v.circular_dim_list)
        at += v.dim
    circ = np.array(circ)
    # a "truth" near a sample, a third of a spread off in every coordinate: inside the posterior
    truth_of = {v: host[3, cols[v]].astype(np.float64) + 0.3 * host[:, cols[v]].astype(np.float64).std(axis=0) for v in order}
    points = {order[0]: host[:7, cols[order[0]]].astype(np.float64), pair: np.hstack([host[:5, cols[pair[0]]], host[:5, cols[pair[1]]]])}
    before = solver.posterior_summary(samples=drawn, pairs=[pair])
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
             list(solver.elimination_ordering), len(solver.physical_factors))
    res = solver.posterior_marginal_density(samples=drawn, pairs=[pair], curves=g, maps=(24, 20), at=points, truth=truth_of)
    assert torch.equal(state[0], torch.get_rng_state()) and torch.equal(state[1], torch.cuda.get_rng_state())
    assert np.array_equal(state[2], np.random.get_state()[1]) and state[3] == random.getstate()
    assert state[4] == list(solver.elimination_ordering) and state[5] == len(solver.physical_factors)
    after = solver.posterior_summary(samples=drawn, pairs=[pair])
    for key in ("mean", "cov", "pair_cov"):
        for v in before[key]:
            assert np.array_equal(before[key][v], after[key][v]), (key, v)

    assert set(res) == {"curves", "maps", "log_density", "nlpd", "hpd_level", "mean_nlpd", "coverage", "bandwidth", "n", "ess"}
    assert res["n"] == n and res["ess"] == float(n) and set(res["bandwidth"]) == set(order) | {pair}
    # the bandwidths are density_bandwidth of the summary's covariances
    for v in order:
        H = ST.density_bandwidth(before["cov"][v], float(n), v.dim, "scott", circ[cols[v]])
        assert np.array_equal(res["bandwidth"][v]["H"], H) and res["bandwidth"][v]["factor"] == ST.density_factor(float(n), v.dim, "scott")
    # curves: positive, and they integrate to 1 within the mass the +-3 h span leaves out plus the trapezoid rule's error
    for v in order:
        assert len(res["curves"][v]) == v.dim
        for c, curve in enumerate(res["curves"][v]):
            xs, dens, h = curve["x"], curve["density"], curve["h"]
            assert xs.shape == (g,) and dens.shape == (g,) and np.all(dens >= 0) and np.all(np.diff(xs) > 0)
            col = host[:, cols[v][c]]
            if circ[cols[v][c]]:
                assert xs[0] == np.float32(-np.pi) and xs[-1] < np.pi
                step = 2 * np.pi / g
                total = float(dens.sum() * step)                    # the periodic trapezoid rule
                span, left_out = 2 * np.pi, gaussian_tail(np.pi / h)  # the nearest image: a kernel's mass beyond half a turn
            else:
                z_lo, z_hi = (float(col.min()) - xs[0]) / h, (xs[-1] - float(col.max())) / h     # (the grid is rounded to float32)
                assert z_lo >= 2.99 and z_hi >= 2.99
                step = float(np.diff(xs).max())
                total = float(np.sum(0.5 * (dens[1:] + dens[:-1]) * np.diff(xs)))
                span, left_out = float(xs[-1] - xs[0]), 0.5 * (gaussian_tail(z_lo) + gaussian_tail(z_hi))
            bound = left_out + step ** 2 / 12.0 * 0.4 / h ** 3 * span + 1e-6
            print(v.name, c, "curve integral", total, "bound on |1 - integral|", bound, "h", h, "step / h", step / h)
            assert abs(1.0 - total) <= bound and total <= 1.0 + step ** 2 / 12.0 * 0.4 / h ** 3 * span + 1e-6
            # and a curve is the 1-D density of that column under its own bandwidth
            W = np.array([[1.0 / h]])
            ref, b = oracle_log_density(xs.astype(np.float32).reshape(-1, 1), col.reshape(-1, 1), [0], [0], W, [int(circ[cols[v][c]])],
                                        exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(n))
            assert np.all(np.abs(np.log(np.maximum(dens, 1e-300)) - ref)[dens > 1e-290] <= (2 * b + 64 * U * (np.abs(ref) + 1))[dens > 1e-290])
    # maps: [gy, gx], the xy block's density; its Riemann sum is near 1
    for v in order:
        mp_ = res["maps"][v]
        assert mp_["density"].shape == (20, 24) and mp_["x"].shape == (24,) and mp_["y"].shape == (20,)
        assert np.allclose(mp_["H"], ST.density_bandwidth(before["cov"][v][:2, :2], float(n), 2, "scott"), rtol=1e-12, atol=0)
        W = ST.density_whiten(mp_["H"])
        grid = np.stack([np.tile(mp_["x"], 20), np.repeat(mp_["y"], 24)], axis=1).astype(np.float32)
        ref, b = oracle_log_density(grid, host[:, cols[v][:2]], [0, 1], [0, 1], W, None, exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(n))
        got = np.log(np.maximum(mp_["density"].reshape(-1), 1e-300))
        ok = mp_["density"].reshape(-1) > 1e-290
        assert np.all(np.abs(got - ref)[ok] <= (2 * b + 64 * U * (np.abs(ref) + 1))[ok])
        mass = float(mp_["density"].sum() * (mp_["x"][1] - mp_["x"][0]) * (mp_["y"][1] - mp_["y"][0]))
        print(v.name, "map mass", mass)
        assert 0.8 < mass < 1.2
    # at: the whole block, heading included, and the pair as one joint block -- the oracle's on the same matrix
    for key, p in points.items():
        blk = key if isinstance(key, tuple) else (key,)
        xc = sum((cols[v] for v in blk), [])
        W = ST.density_whiten(res["bandwidth"][key]["H"])
        ref, b = oracle_log_density(p.astype(np.float32), host, list(range(len(xc))), xc, W, circ[xc].astype(np.uint8),
                                    exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(n))
        _, b_np = oracle_log_density(p.astype(np.float32), host, list(range(len(xc))), xc, W, circ[xc].astype(np.uint8))
        ratio = _note("solver_at", np.abs(res["log_density"][key] - ref), b + b_np)
        assert res["log_density"][key].shape == (p.shape[0],) and np.all(np.abs(res["log_density"][key] - ref) <= b + b_np), (key, ratio)
    # truth: nlpd and hpd_level equal the oracle's on the same matrix; coverage is consistent
    levels = []
    for v in order:
        xc = cols[v]
        W = ST.density_whiten(res["bandwidth"][v]["H"])
        t32 = truth_of[v].astype(np.float32).reshape(1, -1)
        kw = dict(exp_ulp=EXP_ULP, log_ulp=LOG_ULP, depth=depth(n))
        ref, b = oracle_log_density(t32, host, list(range(v.dim)), xc, W, circ[xc].astype(np.uint8), **kw)
        _, b_np = oracle_log_density(t32, host, list(range(v.dim)), xc, W, circ[xc].astype(np.uint8))
        assert abs(res["nlpd"][v] + ref[0]) <= b[0] + b_np[0], v
        own, bo = oracle_log_density(host, host, xc, xc, W, circ[xc].astype(np.uint8), **kw)
        _, bo_np = oracle_log_density(host, host, xc, xc, W, circ[xc].astype(np.uint8))
        sure_in = np.sum(own - (bo + bo_np) >= ref[0] + b[0] + b_np[0]) / n          # samples surely at least as dense as the truth
        maybe_in = np.sum(own + (bo + bo_np) >= ref[0] - b[0] - b_np[0]) / n
        print(v.name, "nlpd", res["nlpd"][v], "hpd level", res["hpd_level"][v], "oracle", ST.hpd_level(own, ref[0]))
        assert sure_in <= res["hpd_level"][v] <= maybe_in and sure_in == maybe_in, v      # (no sample is within the bounds of a tie)
        assert 0.0 <= res["hpd_level"][v] <= 1.0
        levels.append(res["hpd_level"][v])
    assert min(levels) < 1.0                                          # (some truth lies inside its posterior's samples)
    assert abs(res["mean_nlpd"] - np.mean([res["nlpd"][v] for v in order])) <= 1e-12 * (1 + abs(res["mean_nlpd"]))
    assert set(res["coverage"]) == {0.5, 0.9, 0.95}
    for lev, share in res["coverage"].items():
        assert share == np.mean(np.array(levels) <= lev)
    assert res["coverage"][0.5] <= res["coverage"][0.9] <= res["coverage"][0.95] <= 1.0

    torch.manual_seed(17)
    lying = solver.posterior_marginal_density(n=n, variables=[order[0]], truth=truth_of, bandwidth="loo")   # the draw where it lies
    assert set(lying["nlpd"]) == {order[0]} and lying["curves"] is None and lying["maps"] is None and lying["log_density"] is None
    again = solver.posterior_marginal_density(samples=drawn, variables=[order[0]], truth=truth_of, bandwidth="loo")
    assert lying["nlpd"] == again["nlpd"] and lying["hpd_level"] == again["hpd_level"]
    assert lying["bandwidth"][order[0]]["factor"] <= ST.density_factor(float(n), order[0].dim, "scott") * 2.0
    w = np.random.RandomState(3).uniform(0.5, 1.5, n)
    weighted = solver.posterior_marginal_density(samples=drawn, variables=[order[0]], weights=w, at={order[0]: points[order[0]]})
    assert abs(weighted["ess"] - w.sum() ** 2 / (w * w).sum()) < 1e-9 and np.all(np.isfinite(weighted["log_density"][order[0]]))
    print("largest error / bound so far:", json.dumps(_worst))
