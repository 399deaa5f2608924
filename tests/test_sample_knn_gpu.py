"""nfisam_sample_knn / nfisam_sample_ball_count and the estimators on them against the float64 numpy oracle of
test_sample_knn_cpu.py (brute-force distances, stable argsort, counts).

MAX NORM: distances equal bit for bit, indices and counts equal exactly -- the float64 difference of two float32 values is
    exact, then there is one rounding by `scale` and no sum, so device and numpy must agree.
L2: |dist_dev - dist_ref| <= (d + 2) u dist_ref, u = 2^-53: the squared distance is a sum of d non-negative products, its error
    at most (d + 1) u relative in any order, with or without FMA contraction; the root halves that and adds one rounding.
    Indices equal, except at a query where two of the oracle's k + 1 smallest squared distances lie within 4 (d + 1) u relative
    of each other without being equal (exact ties are never excused: both sides compute them with the same operations and
    break them by j); at most 1 % of a case's queries may be excused, and the inputs here excuse none.
    Counts: every point whose oracle distance is further than (d + 2) u relative from the radius is counted alike.
log_sum: against math.fsum of mpmath logs of the DEVICE's own k-th distances; bound u (m + sum_i |log eps_i|) (2 LOG_ULP + depth),
    LOG_ULP the largest ulp error of the device's log over the tests' distances against mpmath (measured by
    `device_log_ulp` -- a 1 x 1 point set with one block per distance, whose scale IS the distance, so that log_sum[b] is the
    device's log of it -- asserted here to hold, recorded in profiles/knn.json by scripts/sample_knn.py --tests), depth the
    additions a term goes through: a thread's ceil(m / 256) - 1, the shuffle tree's 6, the waves' 3.
n_used: exact."""
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
from test_sample_knn_cpu import (bivariate, gaussian, oracle_count, oracle_dist, oracle_entropy, oracle_knn, oracle_log_sum,
                                 oracle_mutual_information, poses, ring, standardising_scale)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
U = 2.0 ** -53
LOG_ULP = 1.7          # the device's float64 log against mpmath over these tests' distances (measured: 1.64): see the head comment
_worst = {}


def _note(kind, err, bound):
    ratio = float(np.max(np.asarray(err, dtype=np.float64) / np.asarray(bound, dtype=np.float64))) if np.size(err) else 0.0
    _worst[kind] = max(_worst.get(kind, 0.0), ratio)
    return ratio


def depth(m):
    return (m + 255) // 256 - 1 + 6 + 3


def mp_log_sum(eps):
    """(math.fsum of the mpmath logs of the positive finite eps, how many, sum of |log|)."""
    used = eps[(eps > 0) & np.isfinite(eps)]
    logs = [float(mpmath.log(mpmath.mpf(float(e)))) for e in used]
    return math.fsum(logs), len(logs), math.fsum(abs(v) for v in logs)


def device_log_ulp(eps):
    """The largest error, in ulps of the result, of the device's log over the positive finite values of eps: x = 0 and y = 1,
    one block per value with the value as its scale: dist = eps exactly, and log_sum[b] is a sum of that one term."""
    eps = np.unique(eps[(eps > 0) & np.isfinite(eps)])[:60000]
    if eps.size == 0:
        return 0.0
    one = np.zeros(eps.size, dtype=np.int32)
    out = nh.sample_knn(np.zeros((1, 1), dtype=np.float32), np.ones((1, 1), dtype=np.float32), nh.pack_knn_blocks(np.ones(eps.size)),
                        one, one, k=1, scale=eps, device=DEV)
    assert np.array_equal(out["dist"].cpu().numpy().reshape(-1), eps)
    got = out["log_sum"].cpu().numpy()
    worst = 0.0
    with mpmath.workprec(120):
        for e, g in zip(eps, got):
            exact = mpmath.log(mpmath.mpf(float(e)))
            ulp = math.ulp(float(exact)) if float(exact) != 0.0 else 2.0 ** -1074
            worst = max(worst, float(abs(mpmath.mpf(float(g)) - exact) / ulp))
    _worst["device_log_ulp"] = max(_worst.get("device_log_ulp", 0.0), worst)
    return worst


def _tables(specs, radius_rows=None):
    """specs: [(xcols, ycols, scale [d] or None, wrap [d])] -> (blocks, xcols, ycols, scale, wrap), every block its own entries."""
    blocks = nh.pack_knn_blocks([len(s[0]) for s in specs], radius_rows)
    xc = np.concatenate([np.asarray(s[0]) for s in specs]).astype(np.int32)
    yc = np.concatenate([np.asarray(s[1]) for s in specs]).astype(np.int32)
    scale = np.concatenate([np.ones(len(s[0])) if s[2] is None else np.asarray(s[2], dtype=np.float64) for s in specs])
    wrap = np.concatenate([np.asarray(s[3]) for s in specs]).astype(np.uint8)
    return blocks, xc, yc, scale, wrap


CIRC5 = np.array([0, 0, 1, 0, 0], dtype=np.uint8)


def pose_specs(x, rng):
    """Blocks of 1, 2, 3, 5 and 16 entries over the 5 columns of poses(): the heading alone (wrapped), xy, the pose, all five
    with their own scales, and 16 entries that repeat columns under random scales."""
    sc = standardising_scale(np.nan_to_num(x), CIRC5)
    wide = rng.randint(0, 5, size=16)
    return [([2], [2], None, [1]), ([0, 1], [0, 1], sc[[0, 1]], [0, 0]), ([0, 1, 2], [0, 1, 2], sc[[0, 1, 2]], [0, 0, 1]),
            ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], sc, CIRC5), (wide, wide, sc[wide] * rng.uniform(0.5, 2.0, 16), CIRC5[wide])]


def check_knn(tag, x, y, specs, got, k, norm, exclude_self, b0=0):
    """Blocks b0 .. of the device result `got` (numpy) against the oracle, under the bounds of the head comment."""
    m = x.shape[0]
    all_eps = []
    for b, (xc, yc, scale, wrap) in enumerate(specs):
        d = len(xc)
        D = oracle_dist(x, y, xc, yc, scale, wrap, norm)
        dist, idx = oracle_knn(D, k, exclude_self)
        gd, gi = got["dist"][b0 + b], got["idx"][b0 + b]
        assert gd.shape == (k, m) and gi.shape == (k, m) and gi.dtype == np.int32
        assert np.array_equal(np.isinf(gd), np.isinf(dist)) and not np.isnan(gd).any(), (tag, b)
        if norm == "max":
            assert np.array_equal(gd, dist), (tag, b, np.abs(gd - dist)[np.isfinite(dist)].max())
            assert np.array_equal(gi, idx), (tag, b)
        else:
            fin = np.isfinite(dist)
            bound = (d + 2) * U * dist[fin]
            err = np.abs(gd[fin] - dist[fin])
            live = bound > 0
            ratio = _note("l2_distance", err[live], bound[live])
            assert np.all(err <= bound), (tag, b, ratio)
            D2, _ = oracle_knn(oracle_dist(x, y, xc, yc, scale, wrap, norm, squared=True), k + 1, exclude_self)
            lo, hi = D2[:-1], D2[1:]
            with np.errstate(invalid="ignore"):
                near = (np.isfinite(hi) & (hi != lo) & (hi - lo <= 4 * (d + 1) * U * hi)).any(axis=0)
            wrong = (gi != idx).any(axis=0)
            print(tag, "block", b, "l2 distance error / bound", ratio, "excused queries", int(near.sum()), "of", m)
            assert not np.any(wrong & ~near), (tag, b, np.flatnonzero(wrong & ~near)[:5])
            assert near.sum() <= 0.01 * m, (tag, b, int(near.sum()))
        # log_sum and n_used, from the device's own k-th distances
        ref, used, mag = mp_log_sum(gd[k - 1])
        assert int(got["n_used"][b0 + b]) == used == oracle_log_sum(dist[k - 1])[1], (tag, b)
        bound = U * (m + mag) * (2.0 * LOG_ULP + depth(m))
        ratio = _note("log_sum", abs(got["log_sum"][b0 + b] - ref), bound)
        assert abs(got["log_sum"][b0 + b] - ref) <= bound, (tag, b, ratio)
        all_eps.append(gd[k - 1])
    return np.concatenate(all_eps)


def run_knn(x, y, specs, k, norm, exclude_self):
    blocks, xc, yc, scale, wrap = _tables(specs)
    out = nh.sample_knn(x, y, blocks, xc, yc, k=k, norm=norm, scale=scale, wrap=wrap, exclude_self=exclude_self, device=DEV)
    return {key: v.cpu().numpy() for key, v in out.items()}


# ---- 1. neighbours ----------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, True), (63, 63, True), (64, 64, True), (65, 65, True), (200, 200, True), (65, 200, False), (200, 63, False)]


@pytest.mark.parametrize("norm", ["max", "l2"])
@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("m, n, exclude_self", SHAPES)
def test_neighbours_match_the_oracle(m, n, exclude_self, k, norm):
    """Blocks of 1, 2, 3, 5 and 16 entries, a heading that straddles +-pi; m = n with the pair j == i left out (n - 1 < k: +inf /
    -1 slots), and two sets."""
    x = poses(m, 100 + m)
    y = x if exclude_self else poses(n, 300 + n)
    specs = pose_specs(x, np.random.RandomState(m + n + k))
    got = run_knn(x, None if exclude_self else y, specs, k, norm, exclude_self)
    eps = check_knn("m %d n %d k %d %s" % (m, n, k, norm), x, y, specs, got, k, norm, exclude_self)
    if n - (1 if exclude_self else 0) < k:
        assert np.isinf(got["dist"][:, k - 1]).all() and (got["idx"][:, k - 1] == -1).all() and not got["n_used"].any()
        assert np.all(got["log_sum"] == 0.0)
    worst = device_log_ulp(eps)
    print("device log: largest error", worst, "ulp over", eps.size, "distances")
    assert worst <= LOG_ULP


@pytest.mark.parametrize("norm", ["max", "l2"])
def test_duplicates_ties_and_a_nan_coordinate(norm):
    """20 rows are copies of others (exact ties broken by j, eps = 0 for k = 1: left out of log_sum), row 5 has a NaN x: as a
    query it gets +inf / -1 in every block that reads x, as a point it is nobody's neighbour there."""
    x = poses(200, 9, nan_at=5, dup=20)
    specs = pose_specs(x, np.random.RandomState(2))
    for k in (1, 4):
        got = run_knn(x, None, specs, k, norm, True)
        check_knn("dup k %d %s" % (k, norm), x, x, specs, got, k, norm, True)
        for b in (1, 2, 3):                                        # the blocks that read column 0
            assert np.isinf(got["dist"][b][:, 5]).all() and (got["idx"][b][:, 5] == -1).all() and not (got["idx"][b] == 5).any()
        assert np.isfinite(got["dist"][0][:, 5]).all()             # the heading block does not
        if k == 1:
            zeros = (got["dist"][:, 0] == 0).sum(axis=1)
            # 19 pairs of copies (row 194 copies row 5 as it was before the NaN): 38 zeros; the heading block sees all 20 pairs
            assert np.all(zeros[[1, 2, 3]] == 38) and np.all(got["n_used"][[1, 2, 3]] == 200 - 38 - 1), (zeros, got["n_used"])
            assert zeros[0] == 40 and got["n_used"][0] == 160
            assert got["idx"][3][0, 0] == 199 and got["idx"][3][0, 199] == 0
    y = np.repeat(poses(8, 4), 3, axis=0)                          # every point three times: ties by ascending j
    got = run_knn(y[:5], y, specs[1:2], 4, norm, False)
    assert np.array_equal(got["idx"][0][:3, 0], [0, 1, 2]) and np.all(got["dist"][0][:3, 0] == 0)
    check_knn("triples " + norm, y[:5], y, specs[1:2], got, 4, norm, False)


# ---- 2. counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["max", "l2"])
@pytest.mark.parametrize("m, n, exclude_self", SHAPES)
def test_ball_counts_match_the_oracle(m, n, exclude_self, norm):
    """Radius rows: the 4th (or last) distance of the widest block, a constant, and one with a NaN, a negative, a zero and an
    infinite radius."""
    x = poses(m, 100 + m, dup=3)
    y = x if exclude_self else poses(n, 300 + n)
    specs = pose_specs(x, np.random.RandomState(m + n))
    kk = min(4, n - (1 if exclude_self else 0))
    eps = oracle_knn(oracle_dist(x, y, *specs[3], norm), max(kk, 1), exclude_self)[0][max(kk, 1) - 1]
    odd = np.resize(np.array([np.nan, -1.0, 0.0, np.inf, 0.5]), m)
    radius = np.stack([eps, np.full(m, 0.7), odd])
    rows = [0, 1, 2, 0, 1]
    blocks, xc, yc, scale, wrap = _tables(specs, rows)
    got = nh.sample_ball_count(x, None if exclude_self else y, blocks, xc, yc, radius, norm=norm, scale=scale, wrap=wrap,
                               exclude_self=exclude_self, device=DEV).cpu().numpy()
    assert got.shape == (len(specs), m) and got.dtype == np.int32
    for b, (sx, sy, sc, wr) in enumerate(specs):
        D, r = oracle_dist(x, y, sx, sy, sc, wr, norm), radius[rows[b]]
        ref = oracle_count(D, r, exclude_self)
        if norm == "max":
            assert np.array_equal(got[b], ref), (b, np.flatnonzero(got[b] != ref)[:5])
        else:
            tol = (len(sx) + 2) * U                                # (D (1 + tol) < r: surely inside; D (1 - tol) >= r: surely not)
            lo, hi = oracle_count(D, r / (1 + tol), exclude_self), oracle_count(D, r / (1 - tol), exclude_self)
            assert np.all((lo <= got[b]) & (got[b] <= hi)), b
        bad = ~(r >= 0)
        assert not got[b][bad].any()
    if m >= 4:
        assert got[2][3] == n - (1 if exclude_self else 0)         # an infinite radius: every other point


# ---- 3. the promises: same bits twice, anywhere in a table, repeated, overlapping; a query does not depend on m -----------------
@pytest.mark.parametrize("norm", ["max", "l2"])
def test_table_invariance(norm):
    x, y = poses(130, 7, dup=4), poses(90, 8)
    specs = pose_specs(x, np.random.RandomState(5))
    blocks, xc, yc, scale, wrap = _tables(specs)
    Xt, Yt = nh._columns(x, DEV), nh._columns(y, DEV)
    radius = torch.from_numpy(np.random.RandomState(1).uniform(0.1, 2.0, (2, 130))).to(DEV)
    first = nh.sample_knn_t(Xt, Yt, blocks, xc, yc, 4, norm, scale, wrap)
    again = nh.sample_knn_t(Xt, Yt, blocks, xc, yc, 4, norm, scale, wrap)
    for key in nh.KNN_KEYS:
        assert torch.equal(first[key], again[key]), key
    blocks["radius_row"] = [0, 1, 0, 1, 0]
    cnt = nh.sample_ball_count_t(Xt, Yt, blocks, xc, yc, radius, norm, scale, wrap)
    assert torch.equal(cnt, nh.sample_ball_count_t(Xt, Yt, blocks, xc, yc, radius, norm, scale, wrap))
    # reordered and repeated, and two blocks that overlap the pose block's entries (xy = its first two, the heading its third)
    order = [3, 0, 3, 4, 2, 1, 0]
    table = blocks[order].copy()
    o = int(blocks["col_off"][2])
    extra = np.zeros(2, dtype=nh.KNN_BLOCK_DTYPE)
    extra["col_off"], extra["d"], extra["radius_row"] = [o, o + 2], [2, 1], [1, 0]
    table = np.concatenate([table, extra])
    mixed = nh.sample_knn_t(Xt, Yt, table, xc, yc, 4, norm, scale, wrap)
    mcnt = nh.sample_ball_count_t(Xt, Yt, table, xc, yc, radius, norm, scale, wrap)
    for at, b in enumerate(order):
        for key in nh.KNN_KEYS:
            assert torch.equal(mixed[key][at], first[key][b]), (key, at, b)
        assert torch.equal(mcnt[at], cnt[b]), (at, b)
    # the overlapping blocks equal the same columns listed as blocks of their own (block 1 = xy under the same scales)
    for key in nh.KNN_KEYS:
        assert torch.equal(mixed[key][7], first[key][1]), key
    assert torch.equal(mcnt[7], cnt[1])
    alone = nh.sample_knn_t(Xt, Yt, blocks[2:3].copy(), xc, yc, 4, norm, scale, wrap)
    assert all(torch.equal(alone[key][0], first[key][2]) for key in nh.KNN_KEYS)
    # the first 70 queries alone: the same neighbours (log_sum is a sum over the queries)
    part = nh.sample_knn_t(Xt[:, :70].contiguous(), Yt, blocks, xc, yc, 4, norm, scale, wrap)
    assert torch.equal(part["dist"], first["dist"][:, :, :70]) and torch.equal(part["idx"], first["idx"][:, :, :70])
    pcnt = nh.sample_ball_count_t(Xt[:, :70].contiguous(), Yt, blocks, xc, yc, radius[:, :70].contiguous(), norm, scale, wrap)
    assert torch.equal(pcnt, cnt[:, :70])
    # scale None is scale 1, wrap None is no wrap
    plain = nh.sample_knn_t(Xt, Yt, blocks[1:2].copy(), xc, yc, 4, norm, None, None)
    ones = nh.sample_knn_t(Xt, Yt, blocks[1:2].copy(), xc, yc, 4, norm, np.ones(xc.size), np.zeros(xc.size, dtype=np.uint8))
    assert all(torch.equal(plain[key], ones[key]) for key in nh.KNN_KEYS)


# ---- 4. bad tables -----------------------------------------------------------------------------------------------------------------
def _sentinel(nb, k, m):
    return dict(dist=torch.full((nb, k, m), -7.0, dtype=torch.float64, device=DEV), idx=torch.full((nb, k, m), -7, dtype=torch.int32, device=DEV),
                log_sum=torch.full((nb,), -7.0, dtype=torch.float64, device=DEV), n_used=torch.full((nb,), -7, dtype=torch.int32, device=DEV))


def test_a_bad_block_given_to_the_c_entry_yields_nan_and_leaves_the_others_alone():
    """`checked=True` skips the binding's checks: the C entry sees a row past its matrix, a negative row, blocks that leave
    the entry lists and a radius row past the radii.  The reads stay in bounds by construction (such a block is never walked)."""
    x, y = poses(100, 7), poses(80, 8)
    specs = pose_specs(x, np.random.RandomState(5))[:3]
    blocks, xc, yc, scale, wrap = _tables(specs, [0, 1, 0])
    Xt, Yt = nh._columns(x, DEV), nh._columns(y, DEV)
    radius = torch.from_numpy(np.random.RandomState(1).uniform(0.1, 2.0, (2, 100))).to(DEV)
    good = {key: v.cpu().numpy() for key, v in nh.sample_knn_t(Xt, Yt, blocks, xc, yc, 4, "max", scale, wrap).items()}
    good["count"] = nh.sample_ball_count_t(Xt, Yt, blocks, xc, yc, radius, "max", scale, wrap).cpu().numpy()

    def check(table, cx, cy, bad_block, count_only=False):
        out = {key: v.cpu().numpy() for key, v in nh.sample_knn_t(Xt, Yt, table, cx, cy, 4, "max", scale, wrap, checked=True).items()}
        out["count"] = nh.sample_ball_count_t(Xt, Yt, table, cx, cy, radius, "max", scale, wrap, checked=True).cpu().numpy()
        for key in out:
            for b in range(3):
                if b != bad_block or (count_only and key != "count"):
                    assert np.array_equal(out[key][b], good[key][b], equal_nan=True), (key, b)
        assert np.all(out["count"][bad_block] == -1)
        if not count_only:
            assert np.all(np.isnan(out["dist"][bad_block])) and np.all(out["idx"][bad_block] == -1)
            assert np.isnan(out["log_sum"][bad_block]) and out["n_used"][bad_block] == 0

    for which in ("x", "y"):
        for bad_row in (5, -1):
            cx, cy = xc.copy(), yc.copy()
            (cx if which == "x" else cy)[2] = bad_row              # entry 2 = the second column of block 1 (entries 1..2)
            check(blocks, cx, cy, 1)
            with pytest.raises(ValueError, match="out of range"):  # the binding's own check refuses it
                nh.sample_knn_t(Xt, Yt, blocks, cx, cy, 4, "max", scale, wrap)
    for off in (int(xc.size), -1, int(xc.size) - 2):               # past the lists, before them, running out of them from inside
        past = blocks.copy()
        past["col_off"][2] = off
        check(past, xc, yc, 2)
        with pytest.raises(ValueError, match="leave"):
            nh.sample_knn_t(Xt, Yt, past, xc, yc, 4, "max", scale, wrap)
    for rr in (2, -1):
        past = blocks.copy()
        past["radius_row"][1] = rr                                 # (the host copy must pass the entry: give it a good one)
        dev_blocks = nh.upload(past.view(np.uint8).reshape(-1), device=DEV)[0]
        tabs = nh.upload(xc, yc, device=DEV)
        cnt = torch.full((3, 100), -7, dtype=torch.int32, device=DEV)
        rc = nh.lib().nfisam_sample_ball_count(C.c_void_p(Xt.data_ptr()), 5, 100, C.c_void_p(Yt.data_ptr()), 5, 80, 0,
                                               blocks.ctypes.data_as(C.c_void_p), C.c_void_p(dev_blocks.data_ptr()), 3,
                                               C.c_void_p(tabs[0].data_ptr()), C.c_void_p(tabs[1].data_ptr()), int(xc.size), None, None,
                                               0, C.c_void_p(radius.data_ptr()), 2, C.c_void_p(cnt.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == nh.OK and bool((cnt[1] == -1).all()) and not bool((cnt[[0, 2]] == -7).any())
        with pytest.raises(ValueError, match="radius_row"):
            nh.sample_ball_count_t(Xt, Yt, past, xc, yc, radius, "max", scale, wrap)
    # a device copy with a bad width under a good host copy
    wide = blocks.copy()
    wide["d"][0] = 17
    dev_blocks = nh.upload(wide.view(np.uint8).reshape(-1), device=DEV)[0]
    tabs = nh.upload(xc, yc, device=DEV)
    out = _sentinel(3, 4, 100)
    rc = nh.lib().nfisam_sample_knn(C.c_void_p(Xt.data_ptr()), 5, 100, C.c_void_p(Yt.data_ptr()), 5, 80, 0,
                                    blocks.ctypes.data_as(C.c_void_p), C.c_void_p(dev_blocks.data_ptr()), 3, C.c_void_p(tabs[0].data_ptr()),
                                    C.c_void_p(tabs[1].data_ptr()), int(xc.size), None, None, 4, 0,
                                    *[C.c_void_p(out[key].data_ptr()) for key in nh.KNN_KEYS], None)
    torch.cuda.synchronize()
    assert rc == nh.OK and bool(torch.isnan(out["dist"][0]).all()) and bool((out["idx"][0] == -1).all())
    assert bool(torch.isnan(out["log_sum"][0])) and int(out["n_used"][0]) == 0 and not bool((out["dist"][1:] == -7).any())


def test_what_the_entries_refuse_writes_nothing():
    x = poses(64, 7)
    specs = pose_specs(x, np.random.RandomState(5))[:2]
    blocks, xc, yc, scale, wrap = _tables(specs)
    Xt = nh._columns(x, DEV)
    radius = torch.ones(1, 64, dtype=torch.float64, device=DEV)

    def refused(table=blocks, k=4, norm="max", Yt=None, exclude_self=False, kk=4):
        out = _sentinel(2, kk, 64)
        with pytest.raises(ValueError, match="nfisam_sample_knn"):
            nh.sample_knn_t(Xt, Yt, table, xc, yc, k, norm, scale, wrap, exclude_self, checked=True, out=out)
        cnt = torch.full((2, 64), -7, dtype=torch.int32, device=DEV)
        if k == 4:                                                 # (k is not the count's)
            with pytest.raises(ValueError, match="nfisam_sample_ball_count"):
                nh.sample_ball_count_t(Xt, Yt, table, xc, yc, radius, norm, scale, wrap, exclude_self, checked=True, out=cnt)
        torch.cuda.synchronize()
        assert all(bool((v == -7).all()) for v in out.values()) and bool((cnt == -7).all())

    for value in (0, 17, -2):
        bad = blocks.copy()
        bad["d"][1] = value
        refused(bad)
    refused(k=0, kk=1)
    refused(k=17, kk=17)
    refused(norm=2)
    refused(Yt=Xt[:, :63].contiguous(), exclude_self=True)
    bad = blocks.copy()
    bad["radius_row"][1] = 1
    cnt = torch.full((2, 64), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="nfisam_sample_ball_count"):
        nh.sample_ball_count_t(Xt, None, bad, xc, yc, radius, "max", scale, wrap, checked=True, out=cnt)
    torch.cuda.synchronize()
    assert bool((cnt == -7).all())
    out = _sentinel(2, 4, 64)                                      # and the same call with good arguments writes all of it
    nh.sample_knn_t(Xt, None, blocks, xc, yc, 4, "max", scale, wrap, True, checked=True, out=out)
    nh.sample_ball_count_t(Xt, None, blocks, xc, yc, radius, "max", scale, wrap, True, checked=True, out=cnt)
    assert not any(bool((v == -7).any()) for v in out.values()) and not bool((cnt == -7).any())


# ---- 5. utils.Statistics ---------------------------------------------------------------------------------------------------------
def _log_sum_bound(eps, m):
    """How far the device's log_sum may lie from the oracle's (numpy logs, an ulp each, added by fsum) of the same distances."""
    used = eps[(eps > 0) & np.isfinite(eps)]
    return U * (m + float(np.abs(np.log(used)).sum())) * (2.0 * LOG_ULP + depth(m) + 1.0)


@pytest.mark.parametrize("norm", ["max", "l2"])
def test_statistics_knn_entropy(norm):
    """Equal to the host formula on the oracle's distances under the same scales: H differs by (d / n_used) times the log_sum
    bound plus the formula's own roundings (9 u S, as in the CPU test); for L2 the distances' (d + 2) u moves every log by as
    much: (d / n_used) n_used (d + 2) u more."""
    x = poses(200, 21, dup=6)
    blocks = [[0, 1], [0, 1, 2], [2], [3, 4]]
    circ = CIRC5.astype(bool)
    for given in (x, torch.from_numpy(x).to(DEV)):
        res = ST.knn_entropy(given, blocks, k=4, circular=circ, norm=norm, device=DEV)
        assert set(res) == {"entropy", "n_used", "zeros", "log_sum", "scale", "n", "k", "raw"} and res["n"] == 200 and res["k"] == 4
        used = np.unique(np.concatenate(blocks))
        _, rs, cov = nh.sample_moments(x, nh.pack_moment_blocks(np.ones(used.size)), used, circular=CIRC5[used], device=DEV)
        assert np.array_equal(res["scale"][used], ST.mode_scale(cov.cpu().numpy(), rs.cpu().numpy(), circ[used]))
        assert np.allclose(res["scale"], standardising_scale(x, circ), rtol=1e-12, atol=0)
        for b, cols in enumerate(blocks):
            d = len(cols)
            h, n_used, zeros = oracle_entropy(x, cols, 4, circ, res["scale"], norm)
            eps = res["raw"]["dist"][b, 3].cpu().numpy()
            S = abs(h) + 4 * d + abs(res["log_sum"][b]) * d / n_used + 8
            bound = d / n_used * _log_sum_bound(eps, 200) + 9 * U * S + (d * (d + 2) * U if norm == "l2" else 0.0)
            ratio = _note("entropy", abs(res["entropy"][b] - h), bound)
            print(norm, "block", b, "H", res["entropy"][b], "oracle", h, "error / bound", ratio)
            assert res["n_used"][b] == n_used and res["zeros"][b] == zeros and abs(res["entropy"][b] - h) <= bound
        assert res["zeros"][3] == 0 and res["n_used"][3] == 200
        first = ST.knn_entropy(given, [[0, 1, 2, 3, 4]], k=1, circular=circ, norm=norm, device=DEV)
        assert first["zeros"][0] == 12 and first["n_used"][0] == 188   # the 6 copied rows and their originals
    given = ST.knn_entropy(x, [[0, 1]], k=2, scale=[2.0, 2.0, 0.0, 1.0, 1.0], device=DEV)
    assert np.array_equal(given["scale"], [2.0, 2.0, 0.0, 1.0, 1.0]) and given["k"] == 2
    flat = ST.knn_entropy(np.column_stack([x[:, 0], np.ones(200, dtype=np.float32)]), [[0, 1], [0]], device=DEV)
    assert flat["entropy"][0] == -np.inf and np.isfinite(flat["entropy"][1])          # a column without spread
    # the closed forms, through the device: the oracle's own error on these seeds (test_sample_knn_cpu.py), twice
    xr, true = ring(2000, 21)
    hr = ST.knn_entropy(xr, [[0, 1]], device=DEV)["entropy"][0]
    print("ring, device:", hr, "true", true)
    assert abs(hr - true) <= 2.0 * 0.0521
    xg, true = gaussian(2000, 3, 13)
    assert abs(ST.knn_entropy(xg, [[0, 1, 2]], device=DEV)["entropy"][0] - true) <= 2.0 * 0.0484


def test_statistics_knn_mutual_information():
    """The counts are exact and the formula is the oracle's own: equal to the bit."""
    x = poses(200, 22, dup=5)
    pairs = [([0, 1], [2]), ([0], [1]), ([3], [4]), ([0, 1, 2], [3, 4])]
    circ = CIRC5.astype(bool)
    for given in (x, torch.from_numpy(x).to(DEV)):
        res = ST.knn_mutual_information(given, pairs, k=4, circular=circ, device=DEV)
        assert set(res) == {"mi", "zeros", "scale", "n", "k", "raw"}
        assert np.allclose(res["scale"], standardising_scale(x, circ), rtol=1e-12, atol=0)
        for p, (a, b) in enumerate(pairs):
            mi, n_a, n_b, eps = oracle_mutual_information(x, a, b, 4, circ, res["scale"])
            assert np.array_equal(res["raw"]["eps"][p].cpu().numpy(), eps)
            assert np.array_equal(res["raw"]["count"][2 * p].cpu().numpy(), n_a) and np.array_equal(res["raw"]["count"][2 * p + 1].cpu().numpy(), n_b)
            assert res["mi"][p] == mi and res["zeros"][p] == int((eps == 0).sum())
    xb, true = bivariate(2000, 0.9, 33)
    mi = ST.knn_mutual_information(xb, [([0], [1])], device=DEV)["mi"][0]
    print("rho 0.9, device:", mi, "true", true)
    assert abs(mi - true) <= 2.0 * 0.0506
    with pytest.raises(ValueError, match="norm must be 'max'"):
        ST.knn_mutual_information(x, pairs, norm="l2", device=DEV)


@pytest.mark.parametrize("norm", ["max", "l2"])
def test_statistics_knn_divergence(norm):
    x, y = poses(200, 23), poses(150, 24)
    y[:, 0] += 0.5
    blocks = [[0, 1], ([0, 1, 2], [0, 1, 2]), ([2], [2])]
    circ = CIRC5.astype(bool)
    for gx, gy in ((x, y), (torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))):
        res = ST.knn_divergence(gx, gy, blocks, k=4, circular=circ, norm=norm, device=DEV)
        assert set(res) == {"divergence", "n_used", "scale", "m", "n", "k", "raw"} and (res["m"], res["n"]) == (200, 150)
        for b, blk in enumerate(blocks):
            cols = list(blk[0]) if isinstance(blk, tuple) else blk
            d, sc, wr = len(cols), res["scale"][cols], circ[cols]
            rho = oracle_knn(oracle_dist(x, x, cols, cols, sc, wr, norm), 4, True)[0][3]
            nu = oracle_knn(oracle_dist(x, y, cols, cols, sc, wr, norm), 4, False)[0][3]
            (ls_r, used_r), (ls_n, used_n) = oracle_log_sum(rho), oracle_log_sum(nu)
            ref = ST.divergence_from_log_sums([ls_n], [ls_r], [used_n], [used_r], [d], 200, 150)[0]
            bound = d / 200 * (_log_sum_bound(rho, 200) + _log_sum_bound(nu, 200)) + 6 * U * (abs(ref) + d / 200 * (abs(ls_r) + abs(ls_n)) + 1) + \
                (2 * d * (d + 2) * U if norm == "l2" else 0.0)
            ratio = _note("divergence", abs(res["divergence"][b] - ref), bound)
            print(norm, "block", b, "D", res["divergence"][b], "oracle", ref, "error / bound", ratio)
            assert used_r == used_n == 200 == res["n_used"][b] and abs(res["divergence"][b] - ref) <= bound
    same = ST.knn_divergence(x, x, [[0, 1]], k=1, device=DEV)       # every nu is 0 (the point itself): no query is used
    assert np.isnan(same["divergence"][0]) and same["n_used"][0] == 0


# ---- 6. the solver ----------------------------------------------------------------------------------------------------------------
def test_posterior_information_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem (the fixture and seeds of test_posterior_modes_on_the_small_range_problem)."""
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
    n = 200
    pair = (order[0], order[-1])

    torch.manual_seed(17)
    lying = solver.posterior_information(n=n, pairs=[pair])
    torch.manual_seed(17)
    drawn = solver.posterior_collect(solver.posterior_launch(n))
    before = solver.posterior_summary(samples=drawn, pairs=[pair])
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
             list(solver.elimination_ordering), len(solver.physical_factors))
    given = solver.posterior_information(samples=drawn, pairs=[pair])
    assert torch.equal(state[0], torch.get_rng_state()) and torch.equal(state[1], torch.cuda.get_rng_state())
    assert np.array_equal(state[2], np.random.get_state()[1]) and state[3] == random.getstate()
    assert state[4] == list(solver.elimination_ordering) and state[5] == len(solver.physical_factors)
    after = solver.posterior_summary(samples=drawn, pairs=[pair])
    for key in ("mean", "cov", "pair_cov"):
        for v in before[key]:
            assert np.array_equal(before[key][v], after[key][v]), (key, v)

    assert set(given) == {"entropy", "gaussian_entropy", "negentropy", "mutual_information", "n", "k", "zeros"}
    assert given["n"] == n and given["k"] == 4
    assert set(given["entropy"]) == set(given["gaussian_entropy"]) == set(given["negentropy"]) == set(order)
    assert set(given["mutual_information"]) == {pair} and set(given["zeros"]) == set(order) | {pair}
    for key in ("entropy", "gaussian_entropy", "negentropy", "mutual_information", "zeros"):   # the draw where it lies == handed over
        assert lying[key] == given[key], key

    host = np.hstack([np.asarray(drawn[v], dtype=np.float32) for v in order])
    at, blocks, circ = 0, [], []
    for v in order:
        blocks.append(list(range(at, at + v.dim)))
        circ.extend(bool(c) for c in v.circular_dim_list)
        at += v.dim
    pcols = {v: b for v, b in zip(order, blocks)}
    res = ST.knn_entropy(host, blocks, k=4, circular=circ, device=DEV)
    mi = ST.knn_mutual_information(host, [(pcols[pair[0]], pcols[pair[1]])], k=4, circular=circ, device=DEV)
    assert given["mutual_information"][pair] == mi["mi"][0] and given["zeros"][pair] == mi["zeros"][0]
    for b, v in enumerate(order):
        assert given["entropy"][v] == res["entropy"][b] and given["zeros"][v] == res["zeros"][b], v
        cov = before["cov"][v]
        gauss = 0.5 * (v.dim * np.log(2.0 * np.pi * np.e) + np.linalg.slogdet(cov)[1])
        assert given["gaussian_entropy"][v] == gauss and given["negentropy"][v] == gauss - given["entropy"][v], v
        print(v, "H", given["entropy"][v], "gaussian", gauss, "negentropy", given["negentropy"][v])
        assert np.isfinite(given["entropy"][v]) and np.isfinite(gauss)
    print(pair, "I", given["mutual_information"][pair])
    assert np.isfinite(given["mutual_information"][pair])

    raw = solver.posterior_information(samples=drawn, variables=[order[0]], k=2, standardise=False)
    one = ST.knn_entropy(host, [pcols[order[0]]], k=2, circular=circ, scale=np.ones(host.shape[1]), device=DEV)
    assert raw["entropy"][order[0]] == one["entropy"][0] and raw["k"] == 2 and set(raw["entropy"]) == {order[0]} and not raw["mutual_information"]
    torch.manual_seed(23)
    other = solver.posterior_collect(solver.posterior_launch(150))
    ref = {v: other[v] for v in order[:2]}
    graded = solver.posterior_information(samples=drawn, reference=ref)
    assert set(graded) == set(given) | {"divergence"} and set(graded["divergence"]) == set(order[:2])
    ycols, at = {}, 0
    for v in order[:2]:
        ycols[v] = list(range(at, at + v.dim))
        at += v.dim
    Y = np.hstack([np.asarray(other[v], dtype=np.float32) for v in order[:2]])
    div = ST.knn_divergence(host, Y, [(pcols[v], ycols[v]) for v in order[:2]], k=4, circular=circ, device=DEV)
    for b, v in enumerate(order[:2]):
        print(v, "KL(posterior || second draw)", graded["divergence"][v])
        assert graded["divergence"][v] == div["divergence"][b] and np.isfinite(graded["divergence"][v])
    print("largest error / bound so far:", json.dumps(_worst))
