"""The trajectory-error evaluator on the device against the float64 oracle of tests/test_sample_trajectory_cpu.py (every sum
by math.fsum), and against mpmath at 60 digits where the fit is ill-conditioned.

Shapes: n in {1, 2, 63, 64, 65, 257} (a lane, a tile of 64 samples, one more, five tiles) x P in {1, 2, 3, 63, 64, 65, 257}
(fewer entries than waves, a whole number of rounds of the four waves, one more).  The kernels have no other tile size.

BOUNDS (u = 2^-53; N aligned entries, P entries; kN = ceil(N / 4) + 3 and kP = ceil(P / 4) + 3 are the depths of a sample's
sums: a wave adds every fourth entry in order, then three additions join the waves).  None is fitted to an output; they are
`bounds` of the CPU module.
  rotation   The centroid's error is common to every b' and drops out of dot and cross to first order (sum a' = 0).  Each
             term a'_x b'_x carries the roundings of a', b', and the fma: with the sum, |d dot|, |d cross| <= (kN + 6) u
             sum |a'| |b'| <= (kN + 6) u sqrt(sum |a'|^2 sum |b'|^2), so the angle atan2(cross, dot) moves by at most
             sqrt(2) (kN + 6) u / kappa,  kappa = g / sqrt(sum |a'|^2 sum |b'|^2)  -- the transform's sensitivity: kappa is 1
             for a perfect fit and goes to 0 where dot and cross cancel (a mirrored loop with reflect off).  atan2, sincos and
             the oracle's own roundings add 8 u:   e_rot = (sqrt(2) (kN + 6) / kappa + 8) u,   and 0 where g = 0 exactly (one
             aligned entry, coincident points: b' is exactly 0 on both sides and the rule theta = 0, c = 1 is exact).
             The relative error of the scale g / sum |b'|^2 has the same bound.
  residual   r = a - (c R b + t) with t = a_bar - c R b_bar.  The SAME computed c and R stand in both, so their error acts
             on b - b_bar alone: at most c lever 2 e_rot, lever = max_e |b_e - b_bar| (landmarks included).  The arithmetic
             itself -- two products, a subtraction, the scale, the translation, the difference, for r and again for t, the
             centroid's kN additions, and as much again for the oracle -- is at most 2 (24 + kN) u (1 + c) M, M the largest
             coordinate met (the absolute term: it scales with u max|coord|).   B_res = 2 (24 + kN) u (1 + c) M + 2 c lever e_rot.
  ATE        |sqrt(sse / count) - oracle| <= B_res + 2 kP u ATE: the root mean square of residuals each off by at most B_res
             moves by at most B_res (triangle inequality), and the sum of squares, the division and the root are good to
             2 kP u relative.  The same for landmark_rmse and, with B_res + 4 u value, for the largest residual.
  GUARD      where kappa >= 0.1 and M <= 200 m the asserted ATE bound may not exceed 1e-10 m + 1e-12 ATE (asserted for every
             such sample; the largest B_res among them is 8.3e-12 m, at P = 257 under "similarity").
  theta      e_rot + 4 u pi;   scale: c (e_rot + 4 u);   t: 2 (24 + kN) u (1 + c) M + 2 c |b_bar| e_rot (its lever is b_bar).
  heading    |rms - oracle| <= e_rot + 16 u pi + 2 kP u rms (float32 headings are exact in float64; the sum b_th + theta - a_th
             and the wrap round at pi).
  per entry  sum_i w_i |r_e,i|^2 <= sum_i w_i (2 |r_e,i| B_res,i + B_res,i^2) + (n / 64 + 16) u sum: 6 levels of the shuffle tree,
             the tiles in order, the product with w.
  RPE        trans: |rms - oracle| <= 32 u D + 2 kQ u rms, D the largest |d| of the slot (differences of float32 coordinates
             are exact; sincos, two products and an fma, the truth's rounded difference, the final difference: <= 14 u D on
             the device, as much in the oracle); rot: 32 u pi + 2 kQ u rms; kQ = ceil(pairs / 4) + 3.

Largest measured error / bound on MI355X over every case of this file (printed by `test_report_the_largest_ratios`; kept in
profiles/trajectory_error.json, `largest_ratio`): ate 0.021, landmark_rmse 0.028, largest residual 0.024, theta 0.12, scale
0.15, t 0.035, heading 0.21, per-entry sums 0.018, RPE trans 0.062, RPE rot 0.0083; against mpmath on the ill-conditioned
cases 0.0016 (ate); the solver-level ATE 0.0048.  No bound was exceeded."""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_trajectory_cpu import (SPECIAL, U, bounds, ill_conditioned_cases, mp_trajectory, oracle_rpe, oracle_trajectory,
                                        trajectory_case, wrap_pi)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
NS = [1, 2, 63, 64, 65, 257]
PS = [1, 2, 3, 63, 64, 65, 257]
MODES = ["none", "rigid", "similarity"]

_worst = {}


def _note(kind, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    _worst[kind] = max(_worst.get(kind, 0.0), ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def _case(P):
    return trajectory_case(P)


@functools.lru_cache(maxsize=None)
def _oracle(P, mode, reflect=False):
    x, entries = _case(P)
    o = oracle_trajectory(x, entries, mode, reflect)
    return o, bounds(o, entries)


def _weights(n):
    w = np.random.RandomState(7).uniform(size=257)[:n]
    w[5::10] = 0.0
    return w


def _host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _compare(r, o, b, entries, n, w, label):
    """Every output of one call against the oracle's first n samples."""
    P = entries.size
    kP = -(-P // 4) + 3
    sl = slice(0, n)
    nt, nl, nhd = r["n_traj"], r["n_landmark"], r["n_heading"]
    land = (entries["flags"] & nh.TRAJ_LANDMARK) != 0
    assert (nt, nl, nhd) == (int((~land).sum()), int(land.sum()), int((entries["col_th"] >= 0).sum()))
    for key, sse, cnt in (("ate", "sse_traj", nt), ("landmark_rmse", "sse_landmark", nl)):
        if not cnt:
            assert np.all(r[sse] == 0.0)
            continue
        got, want = np.sqrt(r[sse] / cnt), np.sqrt(o[sse][sl] / cnt)
        bound = b["resid"][sl] + b["rel"] * want
        print(label, key, "ratio", _note(key, np.abs(got - want), bound))
        assert np.all(np.abs(got - want) <= bound), (label, key, np.abs(got - want).max())
        well = (o["kappa"][sl] >= 0.1) & (o["M"][sl] <= 200.0)
        assert np.all(bound[well] <= 1e-10 + 1e-12 * want[well]), (label, key, bound[well].max())       # the guard
    got, want = np.sqrt(r["sse_heading"] / nhd), np.sqrt(o["sse_heading"][sl] / nhd)
    bound = b["heading"][sl] + b["rel"] * want
    print(label, "heading ratio", _note("heading", np.abs(got - want), bound))
    assert np.all(np.abs(got - want) <= bound), (label, np.abs(got - want).max())
    for key, err in (("theta", np.abs(wrap_pi(r["theta"] - o["theta"][sl]))), ("scale", np.abs(r["scale"] - o["scale"][sl])),
                     ("t", np.abs(r["t"].T - o["t"][sl]).max(axis=1))):
        print(label, key, "ratio", _note(key, err, b[key][sl]))
        assert np.all(err <= b[key][sl]), (label, key, err.max())
    assert np.array_equal(r["reflected"].astype(bool), o["reflected"][sl])
    # the largest residual over the trajectory entries, and which entry holds it
    res = np.where(land[None, :], -1.0, o["resid"][sl])
    want = res.max(axis=1)
    bound = b["resid"][sl] + 4 * U * want
    print(label, "worst ratio", _note("worst", np.abs(r["worst"] - want), bound))
    assert np.all(np.abs(r["worst"] - want) <= bound)
    idx = r["worst_entry"]
    assert np.all((idx >= 0) & (idx < P)) and not land[idx].any()
    assert np.all(res[np.arange(n), idx] >= want - 2 * bound)
    # per entry, over the samples
    wv = np.ones(n) if w is None else w
    want = np.array([sum_fs(wv * o["resid"][sl, e] ** 2) for e in range(P)])
    B = b["resid"][sl]
    bound = (wv[:, None] * (2 * o["resid"][sl] * B[:, None] + B[:, None] ** 2)).sum(axis=0) + (n / 64 + 16) * U * want
    print(label, "entry sums ratio", _note("entry_sums", np.abs(r["entry_sums"] - want), bound))
    assert np.all(np.abs(r["entry_sums"] - want) <= bound), (label, np.abs(r["entry_sums"] - want).max())
    assert abs(float(r["weight_sum"]) - sum_fs(wv)) <= (n / 64 + 16) * U * sum_fs(wv)


def sum_fs(v):
    import math
    return math.fsum(np.asarray(v, dtype=np.float64))


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("n", NS)
def test_errors_match_the_float64_oracle(n, P):
    x, entries = _case(P)
    for mode in MODES:
        o, b = _oracle(P, mode)
        for w in (None, _weights(n)):
            r = _host(nh.sample_trajectory_error(x[:n], entries, mode, weights=w, device=DEV))
            _compare(r, o, b, entries, n, w, "n %d P %d %s %s" % (n, P, mode, "w" if w is not None else "-"))
        if mode == "none":
            assert np.all(r["theta"] == 0.0) and np.all(r["scale"] == 1.0) and np.all(r["t"] == 0.0)
            if n > SPECIAL["truth"]:                               # the truth itself: every error exactly 0
                i = SPECIAL["truth"]
                assert r["sse_traj"][i] == 0.0 and r["sse_landmark"][i] == 0.0 and r["sse_heading"][i] == 0.0 and r["worst"][i] == 0.0
        if mode == "similarity" and n > SPECIAL["exact"] and P > 1:    # an exact transform of the truth: recovered
            i = SPECIAL["exact"]
            assert abs(r["theta"][i] - np.pi / 2) <= b["theta"][i] and abs(r["scale"][i] - 2.0) <= b["scale"][i]
            assert np.abs(r["t"][:, i] - [-30.0, 20.0]).max() <= b["t"][i]
            assert np.sqrt(r["sse_traj"][i] / r["n_traj"]) <= b["resid"][i]
        if mode != "none" and (P == 1 or n > SPECIAL["coincident"]):   # the degenerate rule, exactly
            i = 0 if P == 1 else SPECIAL["coincident"]
            assert r["theta"][i] == 0.0 and r["scale"][i] == 1.0 and not r["reflected"][i]
        if P == 1 and mode != "none":
            assert np.all(r["theta"] == 0.0) and np.all(r["scale"] == 1.0)
            assert np.all(np.sqrt(r["sse_traj"]) <= b["resid"][:n])     # one pose: the translation removes its error


@pytest.mark.parametrize("P", [4, 64, 257])
def test_a_mirrored_sample_with_reflect_off_and_on(P):
    """(From three aligned poses on: two points are a segment, which a mirror fits as well as a rotation -- hypot(dot-, cross-)
    equals g and the choice between them is a coin toss of roundings.)"""
    x, entries = _case(P)
    n, i = 65, SPECIAL["mirrored"]
    for mode in ("rigid", "similarity"):
        o_on, b_on = _oracle(P, mode, True)
        on = _host(nh.sample_trajectory_error(x[:n], entries, mode, reflect=True, device=DEV))
        _compare(on, o_on, b_on, entries, n, None, "reflect on P %d %s" % (P, mode))
        assert on["reflected"][i] and np.sqrt(on["sse_traj"][i] / on["n_traj"]) <= b_on["resid"][i]     # ATE ~ 0
        assert np.sqrt(on["sse_heading"][i] / on["n_heading"]) <= b_on["heading"][i]
        assert not on["reflected"][0] and not on["reflected"][SPECIAL["truth"]]
        o_off, b_off = _oracle(P, mode, False)
        off = _host(nh.sample_trajectory_error(x[:n], entries, mode, device=DEV))
        assert not off["reflected"].any()
        # reflect off is the SVD route with d = -1: the oracle (pinned to numpy's SVD in the CPU tests) within the bounds
        assert abs(wrap_pi(off["theta"][i] - o_off["theta"][i])) <= b_off["theta"][i]
        want = np.sqrt(o_off["sse_traj"][i] / off["n_traj"])
        assert abs(np.sqrt(off["sse_traj"][i] / off["n_traj"]) - want) <= b_off["resid"][i] + b_off["rel"] * want
        if P > 4:
            assert want > 1.0


def test_a_nan_or_infinite_coordinate_poisons_its_own_sample_alone():
    P, n = 65, 130
    x, entries = _case(P)
    x = x[:n].copy()
    for mode in MODES:
        clean = _host(nh.sample_trajectory_error(x, entries, mode, device=DEV))
        for bad, col in ((np.nan, 3 * 7 + 1), (np.inf, 3 * 64), (np.nan, 3 * 10 + 2), (-np.inf, 3 * (P - 1))):     # y, x, a heading, a landmark
            y = x.copy()
            y[70, col] = bad
            r = _host(nh.sample_trajectory_error(y, entries, mode, device=DEV))
            for k in ("theta", "scale", "sse_traj", "sse_landmark", "sse_heading", "worst"):
                assert np.isnan(r[k][70]), (mode, col, k)
                assert np.array_equal(np.delete(r[k], 70), np.delete(clean[k], 70)), (mode, col, k)
            assert np.isnan(r["t"][:, 70]).all() and np.array_equal(np.delete(r["t"], 70, axis=1), np.delete(clean["t"], 70, axis=1))
            assert r["worst_entry"][70] == -1 and r["reflected"][70] == 0
            assert np.array_equal(np.delete(r["worst_entry"], 70), np.delete(clean["worst_entry"], 70))
            assert np.isnan(r["entry_sums"]).all()                 # they add over the samples: they follow
            assert float(r["weight_sum"]) == float(clean["weight_sum"])
    pairs = nh.pack_traj_pairs(np.arange(10), [1, 9])
    clean = _host(nh.sample_trajectory_rpe(x, entries, pairs, device=DEV))
    y = x.copy()
    y[70, 3 * 4] = np.nan
    r = _host(nh.sample_trajectory_rpe(y, entries, pairs, device=DEV))
    assert np.isnan(r["trans"][0, 70]) and not np.isnan(r["trans"][1, 70])         # slot 1 = the pair (0, 9) does not read pose 4
    assert np.array_equal(np.delete(r["trans"], 70, axis=1), np.delete(clean["trans"], 70, axis=1))
    assert np.array_equal(r["rot"], clean["rot"])


def test_ill_conditioned_fits_against_mpmath():
    """Graded against the 60-digit values, with the bound the stated sensitivity gives (no guard: kappa is small)."""
    for name, x, entries in ill_conditioned_cases():
        P = entries.size
        for mode in ("rigid", "similarity"):
            o = oracle_trajectory(x, entries, mode)
            b = bounds(o, entries)
            theta, c, t, ate, hrms, _, kappa = mp_trajectory(x[0], entries, mode)
            r = _host(nh.sample_trajectory_error(x, entries, mode, device=DEV))
            got = float(np.sqrt(r["sse_traj"][0] / P))
            print(name, mode, "kappa", kappa, "ate", got, ate, "ratio", _note("ill_ate", abs(got - ate), b["resid"][0] + b["rel"] * ate),
                  "theta ratio", _note("ill_theta", abs(wrap_pi(r["theta"][0] - theta)), b["theta"][0]))
            assert abs(wrap_pi(r["theta"][0] - theta)) <= b["theta"][0]
            assert abs(r["scale"][0] - c) <= b["scale"][0]
            assert max(abs(r["t"][0, 0] - t[0]), abs(r["t"][1, 0] - t[1])) <= b["t"][0]
            assert abs(got - ate) <= b["resid"][0] + b["rel"] * ate
            assert abs(float(np.sqrt(r["sse_heading"][0] / P)) - hrms) <= b["heading"][0] + b["rel"] * hrms


# ---- relative pose error --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3, 63, 64, 65, 257])
@pytest.mark.parametrize("n", NS)
def test_relative_pose_error_matches_the_oracle(n, P):
    x, entries = _case(P)
    poses = np.flatnonzero(entries["col_th"] >= 0)
    strides = sorted({k for k in (1, 2, poses.size - 1) if 1 <= k < poses.size})
    pairs = nh.pack_traj_pairs(poses, strides)
    r = _host(nh.sample_trajectory_rpe(x[:n], entries, pairs, device=DEV))
    trans, rot, D = _rpe_oracle(P, tuple(strides), tuple(poses))
    assert list(r["count"]) == [poses.size - k for k in strides]
    for s, k in enumerate(strides):
        cnt = r["count"][s]
        kQ = -(-cnt // 4) + 3
        got, want = np.sqrt(r["trans"][s] / cnt), np.sqrt(trans[s, :n] / cnt)
        bound = 32 * U * D[s, :n] + 2 * kQ * U * want
        print("n", n, "P", P, "stride", k, "trans ratio", _note("rpe_trans", np.abs(got - want), bound))
        assert np.all(np.abs(got - want) <= bound), (n, P, k, np.abs(got - want).max())
        got, want = np.sqrt(r["rot"][s] / cnt), np.sqrt(rot[s, :n] / cnt)
        bound = 32 * U * np.pi + 2 * kQ * U * want
        print("n", n, "P", P, "stride", k, "rot ratio", _note("rpe_rot", np.abs(got - want), bound))
        assert np.all(np.abs(got - want) <= bound), (n, P, k, np.abs(got - want).max())
    if poses.size > 2 and n >= 63:
        th = x[:n, entries["col_th"][poses]].astype(np.float64)
        assert np.any(np.abs(th[:, 1:] - th[:, :-1]) > np.pi)      # heading differences cross the seam
    if n > SPECIAL["truth"]:
        assert np.all(r["trans"][:, SPECIAL["truth"]] == 0.0) and np.all(r["rot"][:, SPECIAL["truth"]] == 0.0)


@functools.lru_cache(maxsize=None)
def _rpe_oracle(P, strides, poses):
    x, entries = _case(P)
    return oracle_rpe(x, entries, nh.pack_traj_pairs(np.asarray(poses), list(strides)), len(strides))


# ---- the promises -----------------------------------------------------------------------------------------------------------------
KEYS = ("theta", "scale", "t", "sse_traj", "sse_landmark", "sse_heading", "worst", "reflected", "worst_entry")


def test_two_calls_give_the_same_bits_and_a_sample_depends_on_its_own_column_alone():
    P = 65
    x, entries = _case(P)
    w = _weights(257)
    pairs = nh.pack_traj_pairs(np.flatnonzero(entries["col_th"] >= 0), [1, 2, 5])
    for mode, reflect in (("none", False), ("rigid", True), ("similarity", False)):
        a = _host(nh.sample_trajectory_error(x, entries, mode, reflect, weights=w, device=DEV))
        b = _host(nh.sample_trajectory_error(x, entries, mode, reflect, weights=w, device=DEV))
        for k in KEYS + ("entry_sums", "weight_sum"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (mode, k)
        small = _host(nh.sample_trajectory_error(x[:65], entries, mode, reflect, device=DEV))
        for k in KEYS:                                             # the first 65 columns of n = 257 == the n = 65 call
            assert np.array_equal(a[k][..., :65], small[k]), (mode, k)
        perm = np.random.RandomState(3).permutation(257)
        p = _host(nh.sample_trajectory_error(x[perm], entries, mode, reflect, device=DEV))
        for k in KEYS:                                             # a permutation of the samples permutes the outputs
            assert np.array_equal(p[k], a[k][..., perm]), (mode, k)
    a = _host(nh.sample_trajectory_rpe(x, entries, pairs, device=DEV))
    b = _host(nh.sample_trajectory_rpe(x, entries, pairs, device=DEV))
    small = _host(nh.sample_trajectory_rpe(x[:65], entries, pairs, device=DEV))
    p = _host(nh.sample_trajectory_rpe(x[perm], entries, pairs, device=DEV))
    for k in ("trans", "rot"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k][:, :65], small[k]) and np.array_equal(p[k], a[k][:, perm]), k


def test_the_statistics_front_and_the_column_major_entry_agree():
    P = 64
    x, entries = _case(P)
    L = int(((entries["flags"] & nh.TRAJ_LANDMARK) != 0).sum())
    a = np.stack([entries["ax"], entries["ay"]], axis=1)
    n, w = 65, _weights(65)
    pose_cols = np.stack([entries["col_x"], entries["col_y"], entries["col_th"]], axis=1)[:P - L]
    land_cols = np.stack([entries["col_x"], entries["col_y"]], axis=1)[P - L:]
    got = ST.trajectory_error(x[:n], a[:P - L], entries["ath"][:P - L], pose_cols, land_cols, a[P - L:], align="similarity",
                              weights=w, device=DEV)
    Xt = torch.from_numpy(x[:n]).to(DEV).t().contiguous()
    r = _host(nh.sample_trajectory_error_t(Xt, entries, "similarity", weights=w))
    assert np.array_equal(got["ate"], np.sqrt(r["sse_traj"] / (P - L))) and np.array_equal(got["landmark_rmse"], np.sqrt(r["sse_landmark"] / L))
    assert np.array_equal(got["heading_rms"], np.sqrt(r["sse_heading"] / (P - L))) and np.array_equal(got["t"], r["t"].T)
    assert np.array_equal(got["per_entry_rmse"], np.sqrt(r["entry_sums"] / r["weight_sum"])) and got["n"] == n
    assert np.array_equal(got["worst_pose"][0], r["worst_entry"]) and np.array_equal(got["worst_pose"][1], r["worst"])
    rp = ST.relative_pose_error(x[:n], a[:P - L], entries["ath"][:P - L], pose_cols, strides=(1, 3), device=DEV)
    rt = ST.relative_pose_error_t(Xt, entries, np.arange(P - L), strides=(1, 3))
    raw = _host(nh.sample_trajectory_rpe_t(Xt, entries, nh.pack_traj_pairs(np.arange(P - L), [1, 3])))
    for s, k in enumerate((1, 3)):
        assert rp[k]["pairs"] == P - L - k and np.array_equal(rp[k]["trans"], rt[k]["trans"]) and np.array_equal(rp[k]["rot"], rt[k]["rot"])
        assert np.array_equal(rp[k]["trans"], np.sqrt(raw["trans"][s] / (P - L - k)))


# ---- the solver -------------------------------------------------------------------------------------------------------------------
def test_posterior_trajectory_error_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem (the fixture and seeds of `test_posterior_summary_on_the_small_range_problem`),
    n = 300: the device result equals the oracle on the copied-out matrix within the bounds above; the mean trajectory under
    "none" is `posterior_summary`'s translation_rmse over the poses; "importance" gives `posterior_summary`'s ess."""
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
    from utils import Functions as FN
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
    n = 300
    torch.manual_seed(17)
    drawn = solver.posterior_collect(solver.posterior_launch(n))
    poses = [v for v in solver.physical_vars if v.dim == 3 and v in truth]
    lands = [v for v in solver.physical_vars if v.dim == 2 and v in truth]
    assert len(poses) >= 2
    every = poses + lands
    # the copied-out matrix in a layout of this test's own: three columns per variable
    x = np.zeros((n, 3 * len(every)), dtype=np.float32)
    for k, v in enumerate(every):
        x[:, 3 * k:3 * k + v.dim] = np.asarray(drawn[v])
    cols = 3 * np.arange(len(every))
    entries = nh.pack_traj_entries(cols, cols + 1, np.where(np.arange(len(every)) < len(poses), cols + 2, -1),
                                   np.array([np.asarray(truth[v], dtype=np.float64)[:2] for v in every]),
                                   [float(truth[v][2]) if v.dim == 3 else 0.0 for v in every],
                                   landmark=np.arange(len(every)) >= len(poses))
    strides = (1, len(poses) - 1) if len(poses) > 2 else (1,)
    for mode in MODES:
        out = solver.posterior_trajectory_error(truth, samples=drawn, align=mode, strides=strides, threshold=1.0)
        assert out["poses"] == poses and out["landmarks"] == lands and out["n"] == n and out["ess"] == float(n)
        o = oracle_trajectory(x, entries, mode)
        b = bounds(o, entries)
        want = np.sqrt(o["sse_traj"] / len(poses))
        err = np.abs(out["ate"] - want)
        print(mode, "ate", np.quantile(out["ate"], [0.05, 0.5, 0.95]), "ratio", _note("solver_ate", err, b["resid"] + b["rel"] * want))
        assert np.all(err <= b["resid"] + b["rel"] * want)
        if lands:
            want = np.sqrt(o["sse_landmark"] / len(lands))
            assert np.all(np.abs(out["landmark_rmse"] - want) <= b["resid"] + b["rel"] * want)
        want = np.sqrt(o["sse_heading"] / len(poses))
        assert np.all(np.abs(out["heading_rms"] - want) <= b["heading"] + b["rel"] * want)
        assert np.all(np.abs(wrap_pi(out["theta"] - o["theta"])) <= b["theta"]) and np.all(np.abs(out["scale"] - o["scale"]) <= b["scale"])
        assert np.all(np.abs(out["t"] - o["t"]).max(axis=1) <= b["t"]) and out["t"].shape == (n, 2)
        assert set(out["per_pose_rmse"]) == set(every)
        for k, v in enumerate(every):
            want = np.sqrt(np.mean(o["resid"][:, k] ** 2))
            assert abs(out["per_pose_rmse"][v] - want) <= b["resid"].max() + 1e-13 * want
        assert np.all(np.abs(out["worst_pose"]["value"] - o["resid"][:, :len(poses)].max(axis=1)) <= b["resid"] * 2)
        assert np.all(out["worst_pose"]["index"] < len(poses))
        s = out["summary"]
        assert s["n"] == n and s["ess"] == float(n) and s["best"][1] == out["ate"].min() and abs(s["mean"] - out["ate"].mean()) <= 1e-12
        assert s["quantiles"][0.5] == np.quantile(out["ate"], 0.5) and s["below"] == np.mean(out["ate"] < 1.0)
        trans, rot, D = oracle_rpe(x, entries, nh.pack_traj_pairs(np.arange(len(poses)), list(strides)), len(strides))
        assert set(out["rpe"]) == set(strides)
        for sl, k in enumerate(strides):
            cnt = len(poses) - k
            want = np.sqrt(trans[sl] / cnt)
            assert np.all(np.abs(out["rpe"][k]["trans"] - want) <= 32 * U * D[sl] + 16 * U * want)
            want = np.sqrt(rot[sl] / cnt)
            assert np.all(np.abs(out["rpe"][k]["rot"] - want) <= 32 * U * np.pi + 16 * U * want)
        # the posterior mean, graded the reference's way
        m = out["mean_trajectory"]
        summ = solver.posterior_summary(samples=drawn, variables=poses, truth=truth)
        est = np.array([summ["mean"][v][:2] for v in poses])
        ref = np.array([np.asarray(truth[v], dtype=np.float64)[:2] for v in poses])
        if mode == "none":
            print("mean trajectory", m["ate"], summ["translation_rmse"])
            assert abs(m["ate"] - summ["translation_rmse"]) <= 1e-12 * summ["translation_rmse"]
        else:
            R, c, t = FN.kabsch_umeyama(ref, est)
            if mode == "rigid":
                c, t = 1.0, ref.mean(0) - R @ est.mean(0)
            want = np.sqrt(np.mean(np.sum((ref - (c * est @ R.T + t)) ** 2, axis=1)))
            assert abs(m["ate"] - want) <= 1e-12 * max(want, 1.0) and m["ate"] <= summ["translation_rmse"] * (1 + 1e-12)
    # the draw graded where it lies == the same points handed over
    torch.manual_seed(17)
    lying = solver.posterior_trajectory_error(truth, n=n, align="similarity", strides=strides, threshold=1.0)
    for k in ("ate", "heading_rms", "landmark_rmse", "theta", "scale", "t", "reflected"):
        assert np.array_equal(lying[k], out[k], equal_nan=True), k
    imp = solver.posterior_trajectory_error(truth, samples=drawn, weights="importance", strides=())
    summ = solver.posterior_summary(samples=drawn, weights="importance")
    print("ess", imp["ess"], summ["ess"])
    assert imp["ess"] == summ["ess"] and imp["rpe"] == {} and abs(imp["summary"]["ess"] - imp["ess"]) <= 1e-9 * imp["ess"]
    plain = solver.posterior_trajectory_error(truth, samples=drawn, strides=())
    assert np.array_equal(imp["ate"], plain["ate"])                # weights enter the aggregates alone


def test_report_the_largest_ratios():
    """Prints the largest error / bound of every kind met by the tests above (what the module docstring quotes)."""
    print("largest_ratio", json.dumps({k: float("%.3g" % v) for k, v in sorted(_worst.items())}))
    assert all(v <= 1.0 for v in _worst.values())
