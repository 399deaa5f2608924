"""The sample modes on the device, through the C ABI via the binding, against the float64 oracle of
tests/test_sample_modes_cpu.py.

Bounds; none is fitted to an output.  S is the largest |scale_e * coordinate_e| of the block:
  position   where device and oracle applied the same number of shifts:  |scale_e * wrap_e(pos_dev - pos_ref)| <= 1e-12 (1 + S).
             The float64 oracle differs from its longdouble run by at most 1.2e-14 sigma on the fixture (S = 54, bound
             5.5e-11) and by at most 3.2e-14 scaled units on the slow sets (9 ulp of S = 19.7 on the square, bound 2.1e-11;
             both measured and asserted in the CPU file): the bound is 650 times the oracle's own rounding at the least, which
             is left for the device's exp and its order of summation.
  density    |dens_dev - dens_ref| <= 1e-11 dens_ref: every term of the sum is positive (the MMD test's derivation), and the
             exponent moves by 2 inv u du <= 1e-12-ish for a position within the bound above.
  iterations with tol = 1e-7 the counts are equal, except that at most 1 % of the starts may differ, and then by exactly 1 (a
             shift that lands within rounding of the tolerance); those positions agree within 2 tol sigmas.
  merge      the device merge equals the oracle's merge of the DEVICE's converged points and densities in everything: founders,
             labels, mode positions and densities bit for bit, masses exactly (unit weights: k / n) or to 4 n u (weights).
             Against the oracle's own ascent: n_modes, labels, unlabelled and the masses are equal; a mode's position meets
             the position bound when both sides chose the same founder, and lies within `merge` sigmas otherwise (the members
             of a mode end within rounding of one density, the largest may be another member -- the float64 and longdouble
             oracles disagree in the same way --, and any two members are within the merge radius of the founder).
  re-merge   nfisam_sample_modes_merge on an earlier call's points gives the bits of a full call with the same arguments.

`scripts/sample_modes.py --tests` records the largest error / bound over these cases (`largest_ratio` of its JSON)."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_modes_cpu import (BLOCKS, CIRC, MERGE, TOL, bandwidth, data, fixture_modes, oracle_ascent, oracle_merge, ring,
                                   square, wrap_pi)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
U = 2.0 ** -53
_worst = {}


def _note(kind, err, bound):
    ratio = float(np.max(np.asarray(err) / np.asarray(bound))) if np.size(err) else 0.0
    _worst[kind] = max(_worst.get(kind, 0.0), ratio)
    return ratio


def _tables(specs):
    """specs: [(cols, circ, scale [d], inv)] -> (blocks, cols, scale, wrap), every block with its own entries."""
    blocks = nh.pack_mmd_blocks([len(s[0]) for s in specs], np.ones(len(specs)))
    blocks["inv_two_sigma2"] = [s[3] for s in specs]
    cols = np.concatenate([np.asarray(s[0]) for s in specs]).astype(np.int32)
    scale = np.concatenate([np.asarray(s[2], dtype=np.float64) for s in specs])
    wrap = np.concatenate([np.asarray(s[1]) for s in specs]).astype(np.uint8)
    return blocks, cols, scale, wrap


def _run(x, specs, weights=None, **kw):
    """-> per block dict of numpy arrays (pos [n, d], dens, iters, labels [n], n_modes, mode_pos [max_modes, 16], ...)."""
    blocks, cols, scale, wrap = _tables(specs)
    out = nh.sample_modes(x, blocks, cols, scale=scale, wrap=wrap, weights=weights, device=DEV, **kw)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    res = []
    for b, row in enumerate(blocks):
        o, d = int(row["col_off"]), int(row["d"])
        r = {k: out[k][b] for k in nh.MODE_KEYS if k != "pos"}
        r["pos"] = out["pos"][o:o + d].T.copy()
        res.append(r)
    return res


def _spec(x, cols, circ, weights=None, scale=None):
    sc, inv = bandwidth(x, cols, circ, weights)
    return (cols, circ, sc if scale is None else np.asarray(scale, dtype=np.float64), inv)


def _gap(p, q, circ, scale):
    diff = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    c = np.asarray(circ, dtype=bool)
    diff[..., c] = wrap_pi(diff[..., c])
    return np.abs(diff * scale)


def _S(x, spec):
    return float(np.abs(np.asarray(x, dtype=np.float64)[:, spec[0]] * spec[2]).max())


def _check_points(tag, x, spec, got, ref_pos, ref_dens, rows=None):
    """The strict position and density bounds on the starts `rows` (default: all)."""
    cols, circ, scale, inv = spec
    rows = np.arange(x.shape[0]) if rows is None else rows
    pb = 1e-12 * (1.0 + _S(x, spec))
    gap = _gap(got["pos"][rows], ref_pos[rows], circ, scale)
    ratio = _note("position", gap, pb)
    db = 1e-11 * ref_dens[rows]
    derr = np.abs(got["dens"][rows] - ref_dens[rows])
    live = db > 0
    dratio = _note("density", derr[live], db[live])
    print(tag, "position error / bound", ratio, "density error / bound", dratio)
    assert np.all(gap <= pb), (tag, gap.max(), pb)
    assert np.all(derr <= db), (tag, derr.max())


# ---- 1. a fixed number of iterations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 8, 30])
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_fixed_count_matches_the_oracle(n, iters):
    x, _ = data(n, 5)
    specs = [_spec(x, BLOCKS[name], [CIRC[c] for c in BLOCKS[name]]) for name in ("xy", "pose", "heading")]
    got = _run(x, specs, tol=0.0, max_iters=iters)
    for spec, g in zip(specs, got):
        pos, dens, it = oracle_ascent(x, spec[0], spec[1], spec[2], spec[3], max_iters=iters, tol=0.0)
        assert np.array_equal(np.abs(g["iters"]), np.abs(it)), (n, iters, spec[0])
        _check_points("n %d iters %d block %s" % (n, iters, spec[0]), x, spec, g, pos, dens)


@pytest.mark.parametrize("iters", [1, 8, 30])
def test_fixed_count_on_wide_narrow_repeated_and_unscaled_blocks(iters):
    """d = 16 Gaussians, d = 1, a repeated column, a scale vector with a 0 entry, duplicated rows (rows 0..9 again)."""
    r = np.random.RandomState(31)
    x = (r.randn(130, 16) * np.linspace(0.05, 3.0, 16) + np.linspace(-100.0, 100.0, 16)).astype(np.float32)
    x[120:] = x[:10]
    none16 = [False] * 16
    specs = [_spec(x, list(range(16)), none16), _spec(x, [15], [False]), _spec(x, [3, 3, 8], [False] * 3),
             _spec(x, [0, 1, 2], [False] * 3, scale=[1.0 / 0.05, 0.0, 2.0]), _spec(x, [5, 0, 9, 2, 7], [False] * 5)]
    got = _run(x, specs, tol=0.0, max_iters=iters)
    for spec, g in zip(specs, got):
        pos, dens, it = oracle_ascent(x, spec[0], spec[1], spec[2], spec[3], max_iters=iters, tol=0.0)
        _check_points("iters %d block %s" % (iters, spec[0]), x, spec, g, pos, dens)
        assert np.array_equal(g["pos"][120:], g["pos"][:10]) and np.array_equal(g["dens"][120:], g["dens"][:10])
    # scale 0: the column does not enter the distance -- the ascent in (0, 2) is that of the two columns alone -- and is carried
    # along by the same weights
    two, = _run(x, [((0, 2), [False] * 2, [1.0 / 0.05, 2.0], specs[3][3])], tol=0.0, max_iters=iters)
    assert np.array_equal(got[3]["pos"][:, [0, 2]], two["pos"]) and np.array_equal(got[3]["dens"], two["dens"])
    assert np.array_equal(got[2]["pos"][:, 0], got[2]["pos"][:, 1])               # the repeated column moves as one


@pytest.mark.parametrize("iters", [1, 8, 30])
def test_fixed_count_with_zero_weights_and_a_start_out_of_reach(iters):
    x, _ = data(129, 6)
    x = np.vstack([x, [[1e4, -1e4, 0.5]]]).astype(np.float32)
    w = np.random.RandomState(3).uniform(0.1, 2.0, 130)
    w[7::9] = 0.0
    w[-1] = 0.0
    specs = [_spec(x, BLOCKS[name], [CIRC[c] for c in BLOCKS[name]], w) for name in ("xy", "pose")]
    got = _run(x, specs, weights=w, tol=0.0, max_iters=iters)
    for spec, g in zip(specs, got):
        pos, dens, it = oracle_ascent(x, spec[0], spec[1], spec[2], spec[3], w, max_iters=iters, tol=0.0)
        _check_points("weighted iters %d block %s" % (iters, spec[0]), x, spec, g, pos, dens)
        assert g["iters"][-1] == 0 and g["dens"][-1] == 0.0 and it[-1] == 0       # out of reach: it stays, density 0
        assert np.array_equal(g["pos"][-1], x[-1, spec[0]].astype(np.float64))
        assert np.all(g["iters"][7::9][:-1] != 0)                                 # a zero-weight start in reach climbs


# ---- 2. stopping and merge -----------------------------------------------------------------------------------------------------
def _check_stop_and_merge(tag, x, spec, g, o, weights=None, max_modes=16):
    cols, circ, scale, inv = spec
    n = x.shape[0]
    differ = np.flatnonzero(g["iters"] != o["iters"])
    print(tag, "starts whose iteration count differs:", differ.size, "of", n)
    assert differ.size <= 0.01 * n, (tag, differ.size)
    assert np.all(np.abs(g["iters"][differ] - o["iters"][differ]) == 1)
    if differ.size:
        d2 = 2.0 * inv * (_gap(g["pos"][differ], o["pos"][differ], circ, scale) ** 2).sum(-1)
        assert np.all(np.sqrt(d2) <= 2 * TOL), (tag, np.sqrt(d2).max())
    same = np.flatnonzero(g["iters"] == o["iters"])
    _check_points(tag, x, spec, g, o["pos"], o["dens"], same)
    # the merge of the device's own converged points
    labels, founders, masses, left = oracle_merge(g["pos"], g["dens"], circ, scale, inv, weights, MERGE, max_modes)
    k = len(founders)
    assert g["n_modes"] == k and g["unlabelled"] == left and np.array_equal(g["labels"], labels), tag
    assert np.array_equal(g["mode_pos"][:k, :len(cols)], g["pos"][founders]) and np.array_equal(g["mode_dens"][:k], g["dens"][founders])
    assert np.all(np.isnan(g["mode_pos"][k:])) and np.all(np.isnan(g["mode_dens"][k:])) and np.all(np.isnan(g["mode_mass"][k:]))
    assert np.all(np.isnan(g["mode_pos"][:k, len(cols):]))
    if weights is None:
        assert np.array_equal(g["mode_mass"][:k], masses), (tag, g["mode_mass"][:k], masses)
    else:
        assert np.all(np.abs(g["mode_mass"][:k] - masses) <= 4 * n * U), tag
    assert np.all(np.diff(g["mode_dens"][:k]) <= 0)
    # against the oracle's own ascent
    assert k == len(o["founders"]) and left == o["unlabelled"] and np.array_equal(g["labels"], o["labels"]), tag
    if weights is None:
        assert np.array_equal(g["mode_mass"][:k], o["masses"])
    pb = 1e-12 * (1.0 + _S(x, spec))
    for m in range(k):
        gap = _gap(g["mode_pos"][m, :len(cols)], o["pos"][o["founders"][m]], circ, scale)
        if founders[m] == o["founders"][m] and founders[m] in same:
            assert np.all(gap <= pb), (tag, m, gap)
        else:
            assert np.sqrt(2.0 * inv * (gap ** 2).sum()) <= MERGE, (tag, m, gap)


@pytest.mark.parametrize("n, seed", [(65, 5), (65, 6), (65, 7), (200, 5), (200, 6), (200, 7)])
def test_stopping_and_merge_equal_the_oracle(n, seed):
    x, a = data(n, seed)
    names = ("xy", "pose", "heading")
    fx = [fixture_modes(n, seed, name) for name in names]
    specs = [(f[2], f[3], f[4], f[5]) for f in fx]
    got = _run(x, specs, tol=TOL, merge=MERGE)
    for name, spec, g, f in zip(names, specs, got, fx):
        _check_stop_and_merge("n %d seed %d %s" % (n, seed, name), x, spec, g, f[6])
        assert g["n_modes"] == 2 and g["unlabelled"] == 0
        first = g["labels"][np.flatnonzero(a)[0]]
        assert np.array_equal(g["labels"] == first, a)
        if (n, seed) == (200, 5):
            assert g["mode_mass"][first] == 67 / 200 and g["mode_mass"][1 - first] == 133 / 200
        if name != "xy":                                          # across the seam, not near 0
            h = g["mode_pos"][first, len(spec[0]) - 1]
            assert abs(wrap_pi(np.float64(h - 3.05))) < 0.1 and abs(h) > 2.5
    print("largest error / bound so far:", json.dumps(_worst))


def test_stopping_and_merge_with_weights():
    x, a = data(130, 7)
    w = np.random.RandomState(4).uniform(0.1, 2.0, 130)
    w[3::11] = 0.0
    specs = [_spec(x, BLOCKS[name], [CIRC[c] for c in BLOCKS[name]], w) for name in ("xy", "pose")]
    got = _run(x, specs, weights=w, tol=TOL, merge=MERGE)
    for spec, g in zip(specs, got):
        pos, dens, it = oracle_ascent(x, spec[0], spec[1], spec[2], spec[3], w)
        labels, founders, masses, left = oracle_merge(pos, dens, spec[1], spec[2], spec[3], w)
        o = dict(pos=pos, dens=dens, iters=it, labels=labels, founders=founders, masses=masses, unlabelled=left)
        _check_stop_and_merge("weighted %s" % (spec[0],), x, spec, g, o, weights=w)
        assert abs(g["mode_mass"][:g["n_modes"]].sum() - 1.0) <= 4 * 130 * U


# ---- 3. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_max_iters_max_modes_and_a_constant_block():
    x = square(200, 9)
    spec = _spec(x, [0, 1], [False, False])
    g, = _run(x, [spec], tol=TOL, max_iters=5)
    pos, dens, it = oracle_ascent(x, spec[0], spec[1], spec[2], spec[3], max_iters=5)
    assert (g["iters"] != it).sum() <= 2 and np.all(np.abs(g["iters"] - it)[np.abs(g["iters"]) == np.abs(it)] == 0)
    assert np.all(np.abs(g["iters"]) <= 5) and (g["iters"] < 0).sum() > 100 and (it < 0).sum() > 100
    res = ST.sample_modes(x, [[0, 1]], max_iters=5, device=DEV)
    raw = res["raw"]["iters"][0].cpu().numpy()
    assert res["iterations"]["not_converged"][0] == (raw < 0).sum() > 100 and res["iterations"]["max"][0] == 5

    x, a = data(200, 5)
    spec = _spec(x, BLOCKS["pose"], CIRC)
    g, = _run(x, [spec], max_modes=1)
    assert g["n_modes"] == 1 and g["unlabelled"] in (133, 67) and (g["labels"] == -1).sum() == g["unlabelled"]
    assert g["mode_pos"].shape == (1, 16) and g["mode_mass"][0] == (200 - g["unlabelled"]) / 200
    g32, = _run(x, [spec], max_modes=32)
    assert g32["n_modes"] == 2 and g32["mode_pos"].shape == (32, 16)

    c = np.tile(np.float32([100.25, -3.5, 3.0]), (70, 1))
    for scale in (None, [1.0, 1.0, 1.0]):                         # the default rule (no spread: scale 0), and ones
        g, = _run(c, [_spec(c, [0, 1, 2], CIRC, scale=scale)])
        assert g["n_modes"] == 1 and g["mode_mass"][0] == 1.0 and g["unlabelled"] == 0 and np.all(g["labels"] == 0)
        assert np.array_equal(g["mode_pos"][0, :3], c[0].astype(np.float64)) and np.all(g["pos"] == c.astype(np.float64))
        assert set(g["iters"].tolist()) <= {0, 1} and np.all(g["dens"] == 1.0)


# ---- 4. the same bits alone, repeated, anywhere in a table, and on a second call -----------------------------------------------
def test_table_invariance():
    x, _ = data(200, 6)
    w = np.random.RandomState(8).uniform(0.0, 1.0, 200)
    pose = _spec(x, BLOCKS["pose"], CIRC)
    filler = [_spec(x, BLOCKS["xy"], [False, False]), _spec(x, BLOCKS["heading"], [True])]
    for weights in (None, w):
        alone, = _run(x, [pose], weights)
        again, = _run(x, [pose], weights)
        twice = _run(x, [pose, pose], weights)
        table = _run(x, [pose] + [filler[k % 2] for k in range(38)] + [pose], weights)
        assert len(table) == 40
        for other in (again, twice[0], twice[1], table[0], table[-1]):
            for k in alone:
                assert np.array_equal(alone[k], other[k], equal_nan=True), k
        lone_xy, = _run(x, [filler[0]], weights)
        for k in lone_xy:
            assert np.array_equal(lone_xy[k], table[1][k], equal_nan=True) and np.array_equal(lone_xy[k], table[37][k], equal_nan=True)
    ones, = _run(x, [pose], np.ones(200))                         # NULL weights are all ones
    none, = _run(x, [pose], None)
    for k in none:
        assert np.array_equal(ones[k], none[k], equal_nan=True), k


def test_merge_alone_equals_a_full_call():
    """nfisam_sample_modes_merge on the points of an earlier call: the bits of a full call with the same radius and max_modes,
    and the oracle's merge of those points at another radius."""
    x, _ = data(200, 6)
    w = np.random.RandomState(8).uniform(0.0, 1.0, 200)
    specs = [_spec(x, BLOCKS["pose"], CIRC), _spec(x, BLOCKS["xy"], [False, False])]
    blocks, cols, scale, wrap = _tables(specs)
    Xt = torch.from_numpy(x.T.copy()).to(DEV)
    for weights in (None, w):
        full = nh.sample_modes_t(Xt, blocks, cols, scale, wrap, weights)
        for merge, mm in ((MERGE, 16), (MERGE, 1), (0.5, 32), (1e-4, 3)):
            want = nh.sample_modes_t(Xt, blocks, cols, scale, wrap, weights, merge=merge, max_modes=mm)
            got = nh.sample_modes_merge_t(full, 3, blocks, cols, scale, wrap, weights, merge=merge, max_modes=mm)
            assert got["pos"] is full["pos"] and got["dens"] is full["dens"]
            for k in nh.MODE_KEYS:
                assert torch.equal(got[k], want[k]) or np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=True), (k, merge, mm)
            for b, spec in enumerate(specs):
                o, d = int(blocks[b]["col_off"]), int(blocks[b]["d"])
                labels, founders, masses, left = oracle_merge(full["pos"][o:o + d].T.cpu().numpy().copy(), full["dens"][b].cpu().numpy(),
                                                              spec[1], spec[2], spec[3], weights, merge, mm)
                assert np.array_equal(got["labels"][b].cpu().numpy(), labels) and int(got["unlabelled"][b]) == left
    with pytest.raises(ValueError, match="nfisam_sample_modes_merge"):
        nh.sample_modes_merge_t(full, 3, blocks, cols, scale, wrap, merge=0.0, checked=True)
    with pytest.raises(ValueError, match="merge"):
        nh.sample_modes_merge_t(full, 3, blocks, cols, scale, wrap, merge=0.0)
    with pytest.raises(ValueError, match="belong"):
        nh.sample_modes_merge_t(full, 3, blocks[:1], cols[:3], scale[:3], wrap[:3])


# ---- 5. bad tables -------------------------------------------------------------------------------------------------------------
def _sentinel(ne, nb, n, mm):
    f = dict(pos=((ne, n), torch.float64), dens=((nb, n), torch.float64), iters=((nb, n), torch.int32),
             labels=((nb, n), torch.int32), n_modes=((nb,), torch.int32), mode_pos=((nb, mm, 16), torch.float64),
             mode_dens=((nb, mm), torch.float64), mode_mass=((nb, mm), torch.float64), unlabelled=((nb,), torch.int32))
    return {k: torch.full(shape, -7, dtype=dt, device=DEV) for k, (shape, dt) in f.items()}


def test_a_bad_block_given_to_the_c_entry_yields_nan_and_leaves_the_others_alone():
    """`checked=True` skips the binding's checks: the C entry sees a row past x_rows, a negative row and a block that runs
    past n_entries.  The reads stay in bounds by construction (such a block is never walked)."""
    x, _ = data(100, 7)
    specs = [_spec(x, BLOCKS["xy"], [False, False]), _spec(x, BLOCKS["pose"], CIRC), _spec(x, BLOCKS["heading"], [True])]
    blocks, cols, scale, wrap = _tables(specs)
    Xt = torch.from_numpy(x.T.copy()).to(DEV)
    good = {k: v.cpu().numpy() for k, v in nh.sample_modes_t(Xt, blocks, cols, scale, wrap).items()}

    def check(out, bad_block, pos_rows, orphans=()):
        """pos_rows: the bad block's entries inside the table (NaN); orphans: entries no block owns now (never written)."""
        out = {k: v.cpu().numpy() for k, v in out.items()}
        for k in nh.MODE_KEYS:
            if k == "pos":
                keep = np.ones(cols.size, dtype=bool)
                keep[list(pos_rows) + list(orphans)] = False
                assert np.all(np.isnan(out[k][pos_rows])) and np.array_equal(out[k][keep], good[k][keep])
                continue
            for b in range(3):
                if b != bad_block:
                    assert np.array_equal(out[k][b], good[k][b], equal_nan=True), (k, b)
        assert np.all(np.isnan(out["dens"][bad_block])) and np.all(out["labels"][bad_block] == -1)
        assert out["n_modes"][bad_block] == 0 and out["unlabelled"][bad_block] == 100 and np.all(out["iters"][bad_block] == 0)
        for k in ("mode_pos", "mode_dens", "mode_mass"):
            assert np.all(np.isnan(out[k][bad_block]))

    for bad_row in (3, -1):
        bad = cols.copy()
        bad[3] = bad_row                                          # entry 3 = the second column of block 1 (entries 2..4)
        check(nh.sample_modes_t(Xt, blocks, bad, scale, wrap, checked=True), 1, [2, 3, 4])
        with pytest.raises(ValueError, match="row"):              # the binding's own check refuses it
            nh.sample_modes_t(Xt, blocks, bad, scale, wrap)
    past = blocks.copy()
    past["col_off"][2] = int(cols.size)                           # d = 1: the entry one past the list
    check(nh.sample_modes_t(Xt, past, cols, scale, wrap, checked=True), 2, [], [5])
    past["col_off"][2] = -1
    check(nh.sample_modes_t(Xt, past, cols, scale, wrap, checked=True), 2, [], [5])
    past["col_off"][2] = 5
    # a block that runs past the end from inside: two entries of its own are appended to the lists, the third is missing
    cols8, scale8, wrap8 = np.append(cols, [0, 1]).astype(np.int32), np.append(scale, [1.0, 1.0]), np.append(wrap, [0, 0]).astype(np.uint8)
    past["col_off"][1] = 6
    out = {k: v.cpu().numpy() for k, v in nh.sample_modes_t(Xt, past, cols8, scale8, wrap8, checked=True).items()}
    assert np.all(np.isnan(out["pos"][6:8])) and np.array_equal(out["pos"][[0, 1, 5]], good["pos"][[0, 1, 5]])
    assert np.all(np.isnan(out["dens"][1])) and np.all(out["labels"][1] == -1) and out["n_modes"][1] == 0
    for k in nh.MODE_KEYS[1:]:
        for b in (0, 2):
            assert np.array_equal(out[k][b], good[k][b], equal_nan=True), (k, b)
    with pytest.raises(ValueError, match="leave"):
        nh.sample_modes_t(Xt, past, cols8, scale8, wrap8)


def test_bad_widths_bandwidths_and_scalars_are_refused_by_the_c_entry_and_nothing_is_written():
    x, _ = data(64, 7)
    specs = [_spec(x, BLOCKS["xy"], [False, False]), _spec(x, BLOCKS["pose"], CIRC)]
    blocks, cols, scale, wrap = _tables(specs)
    Xt = torch.from_numpy(x.T.copy()).to(DEV)

    def refused(table=blocks, mm=16, **kw):
        out = _sentinel(int(cols.size), 2, 64, max(mm, 1))
        args = dict(tol=TOL, merge=MERGE, max_iters=10, max_modes=mm)
        args.update(kw)
        with pytest.raises(ValueError, match="nfisam_sample_modes"):
            nh.sample_modes_t(Xt, table, cols, scale, wrap, checked=True, out=out, **args)
        torch.cuda.synchronize()
        for k, v in out.items():
            assert bool((v == -7).all()), k

    for field, value in (("d", 0), ("d", 17), ("d", -2), ("inv_two_sigma2", 0.0), ("inv_two_sigma2", -1.0),
                         ("inv_two_sigma2", np.inf), ("inv_two_sigma2", np.nan)):
        bad = blocks.copy()
        bad[field][1] = value
        refused(bad)
    for kw in (dict(max_iters=0), dict(tol=-1.0), dict(tol=float("nan")), dict(merge=0.0), dict(merge=float("inf")), dict(mm=0),
               dict(mm=33)):
        refused(**kw)
    out = _sentinel(int(cols.size), 2, 64, 16)                    # and the same call with good arguments writes all of it
    nh.sample_modes_t(Xt, blocks, cols, scale, wrap, checked=True, out=out, max_iters=10)
    assert not bool((out["labels"] == -7).any()) and not bool((out["pos"] == -7).any()) and not bool((out["mode_pos"] == -7).any())
    # n == 0: OK, and nothing is touched
    dev = nh.upload(blocks.view(np.uint8).reshape(-1), cols, device=DEV)
    out = _sentinel(int(cols.size), 2, 64, 16)
    rc = nh.lib().nfisam_sample_modes(C.c_void_p(Xt.data_ptr()), 3, 0, blocks.ctypes.data_as(C.c_void_p), C.c_void_p(dev[0].data_ptr()),
                                      2, C.c_void_p(dev[1].data_ptr()), int(cols.size), None, None, None, 10, C.c_double(TOL),
                                      C.c_double(MERGE), 16, *[C.c_void_p(out[k].data_ptr()) for k in nh.MODE_KEYS], None)
    torch.cuda.synchronize()
    assert rc == nh.OK and all(bool((v == -7).all()) for v in out.values())


# ---- 6. utils.Statistics and the solver ------------------------------------------------------------------------------------------
def test_statistics_sample_modes_default_bandwidth_and_device_labels():
    x, a = data(200, 5)
    w = np.random.RandomState(5).uniform(0.2, 1.0, 200)
    for weights in (None, w):
        res = ST.sample_modes(x, [BLOCKS["xy"], BLOCKS["pose"], BLOCKS["heading"]], circular=CIRC, weights=weights, device=DEV)
        for b, name in enumerate(("xy", "pose", "heading")):
            cols = BLOCKS[name]
            sc, inv = bandwidth(x, cols, [CIRC[c] for c in cols], weights)
            assert np.allclose(res["scale"][cols], sc, rtol=1e-12, atol=0) and abs(1 / (2 * res["sigma"][b] ** 2) - inv) <= 1e-12 * inv
            assert len(res["modes"][b]) == 2 and res["unlabelled"][b] == 0 and res["iterations"]["not_converged"][b] == 0
            first = res["labels"][b][np.flatnonzero(a)[0]]
            assert np.array_equal(res["labels"][b] == first, a)
            mass = [m["mass"] for m in res["modes"][b]]
            assert abs(sum(mass) - 1.0) <= 4 * 200 * U and res["modes"][b][0]["density"] >= res["modes"][b][1]["density"]
            assert res["modes"][b][0]["position"].shape == (len(cols),)
            if weights is None:
                assert sorted(mass) == [67 / 200, 133 / 200]
        assert res["n_eff"] == ST.effective_sample_size(weights, 200)
    on_dev = ST.sample_modes(torch.from_numpy(x).to(DEV), [BLOCKS["pose"]], circular=CIRC)
    assert torch.is_tensor(on_dev["labels"]) and on_dev["labels"].is_cuda and on_dev["labels"].dtype == torch.int32
    host = ST.sample_modes(x, [BLOCKS["pose"]], circular=CIRC, device=DEV)
    assert np.array_equal(on_dev["labels"].cpu().numpy(), host["labels"])
    given = ST.sample_modes(x, [BLOCKS["pose"]], circular=CIRC, sigma=0.5, scale=[2.0, 2.0, 0.0], device=DEV)
    assert given["sigma"][0] == 0.5 and np.array_equal(given["scale"], [2.0, 2.0, 0.0])


def test_posterior_modes_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem (the fixture and seeds of the summary's solver test)."""
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
    lying = solver.posterior_modes(n=n, pairs=[pair])
    torch.manual_seed(17)
    drawn = solver.posterior_collect(solver.posterior_launch(n))
    before = solver.posterior_summary(samples=drawn, pairs=[pair])
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
             list(solver.elimination_ordering), len(solver.physical_factors))
    given = solver.posterior_modes(samples=drawn, pairs=[pair])
    assert torch.equal(state[0], torch.get_rng_state()) and torch.equal(state[1], torch.cuda.get_rng_state())
    assert np.array_equal(state[2], np.random.get_state()[1]) and state[3] == random.getstate()
    assert state[4] == list(solver.elimination_ordering) and state[5] == len(solver.physical_factors)
    after = solver.posterior_summary(samples=drawn, pairs=[pair])
    for key in ("mean", "cov", "pair_cov"):
        for v in before[key]:
            assert np.array_equal(before[key][v], after[key][v]), (key, v)

    assert set(given) == {"modes", "pair_modes", "labels", "n", "ess", "sigma", "not_converged", "unlabelled"}
    assert given["n"] == n and given["ess"] == float(n)
    assert set(given["modes"]) == set(given["labels"]) == set(order) and set(given["pair_modes"]) == {pair}
    assert set(given["sigma"]) == set(given["not_converged"]) == set(given["unlabelled"]) == set(order) | {pair}

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(p["position"], q["position"]) and p["mass"] == q["mass"] and
                                        p["density"] == q["density"] for p, q in zip(a, b))
    for v in order:                                               # the device draw where it lies == the same points handed over
        assert same(lying["modes"][v], given["modes"][v]) and torch.equal(lying["labels"][v], given["labels"][v])
    assert same(lying["pair_modes"][pair], given["pair_modes"][pair])

    host = np.hstack([np.asarray(drawn[v], dtype=np.float32) for v in order])
    at, blocks, circ = 0, [], []
    for v in order:
        blocks.append(list(range(at, at + v.dim)))
        circ.extend(bool(c) for c in v.circular_dim_list)
        at += v.dim
    pcols = {v: b for v, b in zip(order, blocks)}
    res = ST.sample_modes(host, blocks + [pcols[pair[0]] + pcols[pair[1]]], circular=circ, device=DEV)
    for b, v in enumerate(order + [pair]):
        modes = given["modes"][v] if v is not pair else given["pair_modes"][pair]
        dim = sum(u.dim for u in v) if v is pair else v.dim
        assert same(modes, res["modes"][b]), v
        assert given["sigma"][v] == res["sigma"][b] == ST.mode_sigma(n, [dim])[0]
        assert given["unlabelled"][v] == res["unlabelled"][b] and given["not_converged"][v] == res["iterations"]["not_converged"][b]
        if v is not pair:
            lab = given["labels"][v]
            assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == (n,)
            assert np.array_equal(lab.cpu().numpy(), res["labels"][b])
        mass = sum(m["mass"] for m in modes)
        print(v, "modes", len(modes), "mass", mass, "unlabelled", given["unlabelled"][v])
        assert len(modes) >= 1 and abs(mass - (1.0 - given["unlabelled"][v] / n)) <= 4 * n * U
        assert all(modes[k]["density"] >= modes[k + 1]["density"] for k in range(len(modes) - 1))
        assert all(m["position"].shape == (dim,) for m in modes)

    w = np.random.RandomState(2).uniform(0.1, 1.0, n)
    wres = solver.posterior_modes(samples=drawn, weights=w, variables=[order[0]], max_modes=2, sigma=0.7)
    assert abs(wres["ess"] - w.sum() ** 2 / (w * w).sum()) <= 1e-12 * n and wres["sigma"][order[0]] == 0.7
    assert len(wres["modes"][order[0]]) <= 2 and set(wres["modes"]) == {order[0]}
    imp = solver.posterior_modes(samples=drawn, weights="importance", variables=[order[0]])
    assert 1.0 <= imp["ess"] <= n and len(imp["modes"][order[0]]) >= 1
    print("largest error / bound so far:", json.dumps(_worst))
