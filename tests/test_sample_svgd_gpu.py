"""The Stein variational direction and step on the GPU (nfisam_sample_svgd, nfisam_sample_step, nfisam_hip.svgd_direction,
utils.Statistics.stein_variational_refine, NFiSAM.posterior_refine / map_refine) against the float64 numpy restatement of
tests/test_sample_svgd_cpu.py across the tile and chunk boundaries, their bitwise promises, and the refinement conditions
of that file's docstring on the device.

Bounds:
  * the direction, |device - numpy| <= TOL (|numpy| + 1) with TOL = 16 x the largest deviation measured on the MI355X
    (DEVICE_MEASURED below, recorded in profiles/svgd.json), at n in {1, 2, 63, 64, 65, 130} over a table of blocks of width
    1, 3, 16, 17 and 33, with and without wrapped columns and a scale = 0 entry.  The launch has one form for every n and width
    (one group per 64 x 64 tile and block): no further n is needed;
  * the step fed the device's own phi: hist within 1e-15 relative (three to four roundings of positive terms), the new points
    within one float32 ulp, 2^-23 |x| (the contraction of the update may differ)."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_svgd_cpu import (EPS, MU, SIGMA, WRAP3, assert_ascent_condition, assert_svgd_conditions, direction,
                                  gaussian_blocks, gaussian_case, step)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEVICE_MEASURED = {"direction": 1.2e-15}                               # (1.13e-15 at n = 65; 6.3e-16 .. 1.03e-15 at the other n > 1)
TOL = {k: 16 * v for k, v in DEVICE_MEASURED.items()}
WIDTHS = (1, 3, 16, 17, 33)


def deviation(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / (np.abs(np.asarray(want)) + 1.0)))


def _random_case(n, D, seed):
    """Points as in tests/test_sample_ksd_gpu.py: offsets to +-50, scores to +-30."""
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, D) * rng.uniform(0.1, 3.0, D) + rng.uniform(-50, 50, D)).astype(np.float32)
    s = rng.randn(n, D) * rng.uniform(0.1, 30.0, D)
    return x, s


def _table_case(n, seed, widths=WIDTHS):
    """A table of blocks of `widths` over a matrix with two more columns than entries, the rows in a shuffled order
    -> (x, xw (the wrapped columns in [-pi, pi], one pair 3.1 / -3.1 across the seam), s, table, cols, scale, scale with a
    zero, wrap)."""
    ne = int(sum(widths))
    x, s = _random_case(n, ne + 2, seed)
    rng = np.random.RandomState(seed + 1)
    cols = rng.permutation(ne + 2)[:ne]
    table = nh.pack_mmd_blocks(widths, np.sqrt(np.asarray(widths, dtype=np.float64)))
    scale = rng.uniform(0.1, 1.0, ne)
    scale0 = scale.copy()
    scale0[np.cumsum(widths) - 1] = 0.0                                # the last entry of every block leaves its kernel
    scale0[0] = scale[0]                                               # (but not the only entry of the block of width 1)
    wrap = np.zeros(ne, dtype=np.uint8)
    wrap[::3] = 1
    xw = x.copy()
    xw[:, cols[wrap != 0]] = rng.uniform(-3.1, 3.1, (n, int(wrap.sum()))).astype(np.float32)
    xw[0, cols[0]] = 3.1
    if n > 1:
        xw[1, cols[0]] = -3.1                                          # a pair across the seam: 0.083 rad apart, not 6.2
    return x, xw, s, table, cols, scale, scale0, wrap


def _host(t):
    return t.cpu().numpy()


# ---- 1. the direction against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 130))
def test_direction_matches_the_numpy_restatement_across_tiles_and_chunks(n):
    x, xw, s, table, cols, scale, scale0, wrap = _table_case(n, 100 * n)
    worst = 0.0
    for pts, sc, wr in ((x, None, None), (xw, scale, wrap), (x, scale0, None), (xw, scale0, wrap)):
        got = nh.svgd_direction(pts, s, table, cols, scale=sc, wrap=wr, device=DEV)
        assert got.dtype == torch.float64 and tuple(got.shape) == (cols.size, n)
        want = direction(pts, s, table, cols, sc, wr)
        assert np.all(np.isfinite(_host(got)))
        worst = max(worst, deviation(_host(got), want))
    if n > 1:                                                          # the wrap matters: the seam pair is in reach only with it
        assert direction(xw, s, table, cols, scale, wrap)[0, 0] != direction(xw, s, table, cols, scale)[0, 0]
    print("n = %3d: |device - numpy| / (|numpy| + 1) = %.3g" % (n, worst))
    assert worst <= TOL["direction"], worst


def test_statistics_direction_fills_the_named_columns():
    x, s = _random_case(65, 7, 9)
    circ = np.zeros(7, dtype=bool)
    circ[5] = True
    x[:, 5] = np.random.RandomState(2).uniform(-3.1, 3.1, 65)
    blocks, scale = [[4, 0], [5], [2, 6, 1]], np.linspace(0.2, 1.0, 7)
    got = ST.stein_variational_direction(x, s, blocks, scale=scale, circular=circ, device=DEV)
    assert got.shape == (65, 7) and got.dtype == np.float64 and np.all(got[:, 3] == 0.0)
    flat = np.concatenate(blocks)
    want = direction(x, s, nh.pack_mmd_blocks([2, 1, 3], np.sqrt([2.0, 1.0, 3.0])), flat, scale[flat], circ[flat])
    assert deviation(got[:, flat].T, want) <= TOL["direction"]
    one = ST.stein_variational_direction(x, s, blocks, sigma=0.5, device=DEV)
    assert deviation(one[:, flat].T, direction(x, s, nh.pack_mmd_blocks([2, 1, 3], [0.5] * 3), flat)) <= TOL["direction"]


# ---- 2. the bitwise promises -----------------------------------------------------------------------------------------------------
def test_bits_on_a_second_call_alone_and_among_others_and_in_both_forms():
    x, xw, s, table, cols, scale, scale0, wrap = _table_case(130, 77, widths=(17, 3, 1))
    a = _host(nh.svgd_direction(xw, s, table, cols, scale=scale0, wrap=wrap, device=DEV))
    b = _host(nh.svgd_direction(xw, s, table, cols, scale=scale0, wrap=wrap, device=DEV))
    assert np.array_equal(a, b)
    # the block of width 17 alone, and last in the table: the same rows of Xt, the same per-entry values, the same bits
    alone = _host(nh.svgd_direction(xw, s, nh.pack_mmd_blocks([17], [np.sqrt(17.0)]), cols[:17], scale=scale0[:17], wrap=wrap[:17],
                                    device=DEV))
    assert np.array_equal(alone, a[:17])
    turn = np.r_[17:21, 0:17]
    last = _host(nh.svgd_direction(xw, s, nh.pack_mmd_blocks([3, 1, 17], np.sqrt([3.0, 1.0, 17.0])), cols[turn], scale=scale0[turn],
                                   wrap=wrap[turn], device=DEV))
    assert np.array_equal(last[4:], a[:17]) and np.array_equal(last[:4], a[17:])
    # the column-major form on the matrices in place, device tensors in the row-major form
    Xt = torch.from_numpy(np.ascontiguousarray(xw.T)).to(DEV)
    Gt = torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV)
    assert np.array_equal(_host(nh.svgd_direction_t(Xt, Gt, table, cols, scale=scale0, wrap=wrap)), a)
    assert np.array_equal(_host(nh.svgd_direction(torch.from_numpy(xw).to(DEV), torch.from_numpy(s).to(DEV), table, cols,
                                                  scale=scale0, wrap=wrap)), a)
    assert np.array_equal(_host(Xt), xw.T)                             # read in place, not written


def test_swapping_the_two_points_of_a_pair_swaps_their_directions():
    """d_ji = -d_ij and k_ji = k_ij to the bit, and the two terms of a point's sum are rounded products: with two points the
    sum is the same bits in either order.  (Among more points the terms are the same bits but their order in the sum is not.)"""
    x, xw, s, table, cols, scale, scale0, wrap = _table_case(2, 31, widths=(33,))
    a = _host(nh.svgd_direction(xw, s, table, cols, scale=scale, wrap=wrap, device=DEV))
    b = _host(nh.svgd_direction(xw[::-1].copy(), s[::-1].copy(), table, cols, scale=scale, wrap=wrap, device=DEV))
    assert np.array_equal(a, b[:, ::-1]) and not np.array_equal(a[:, 0], a[:, 1])


# ---- 3. the step against the restatement, fed the device's own phi ------------------------------------------------------------------
def test_step_matches_the_restatement_and_wraps_into_the_half_open_interval():
    n = 130
    x, xw, s, table, cols, scale, scale0, wrap = _table_case(n, 55, widths=(3, 16, 1))
    xw[:, cols[3]] = np.float32(3.14)                                  # a wrapped column (entry 3) about to cross pi ...
    xw[::2, cols[3]] = np.float32(np.pi)                               # ... half of it from float32(pi) itself
    rng = np.random.RandomState(8)
    eps = rng.uniform(1e-3, 0.5, cols.size)
    hist0 = rng.uniform(0.1, 100.0, (cols.size, n))
    Xt = torch.from_numpy(np.ascontiguousarray(xw.T)).to(DEV)
    Gt = torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV)
    Phi = nh.svgd_direction_t(Xt, Gt, table, cols, scale=scale, wrap=wrap)
    Phi[3] = Phi[3].abs() + 1.0                                        # (upwards, across the seam)
    phi = _host(Phi)
    for first, h_in in ((False, hist0), (True, np.full_like(hist0, np.nan))):
        Xd, hist = Xt.clone(), torch.from_numpy(h_in).to(DEV)
        assert nh.sample_step_t(Xd, cols, Phi, hist, eps, wrap=wrap, alpha=0.9, fudge=1e-6, first=first) is None
        want_x, want_h = step(xw, cols, phi, h_in, eps, wrap, 0.9, 1e-6, first=first)
        got_x, got_h = _host(Xd).T, _host(hist)
        d_h = float(np.max(np.abs(got_h - want_h) / want_h))
        d_x = float(np.max(np.abs(got_x.astype(np.float64) - want_x.astype(np.float64)) / np.maximum(np.abs(want_x), 1e-30)))
        print("first = %s: hist relative %.3g, points relative %.3g (one float32 ulp: %.3g)" % (first, d_h, d_x, 2.0 ** -23))
        assert d_h <= 1e-15 and d_x <= 2.0 ** -23
        if first:
            assert np.array_equal(got_h, phi * phi)                    # the old hist (NaN) is ignored
        seam = got_x[:, cols[3]].astype(np.float64)
        assert np.all(seam < 0) and np.all(seam >= -np.pi) and np.all(seam < np.pi)
        untouched = np.setdiff1d(np.arange(xw.shape[1]), cols)
        assert np.array_equal(got_x[:, untouched], xw[:, untouched])
    moved = np.abs(got_x[:, cols].astype(np.float64) - xw[:, cols]) > 0
    assert moved.mean() > 0.9


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------------
def _gaussian_score_t(Xt):
    mu = torch.tensor(MU, dtype=torch.float64, device=Xt.device)[:, None]
    d = Xt.double() - mu
    d[2] = torch.remainder(d[2] + np.pi, 2.0 * np.pi) - np.pi
    return (-d / torch.tensor(SIGMA ** 2, dtype=torch.float64, device=Xt.device)[:, None]).contiguous()


def test_loop_is_the_manual_calls_and_leaves_the_bits_alone_at_zero_steps():
    start, scale = gaussian_case(65)
    blocks = gaussian_blocks(True)
    flat = np.concatenate(blocks)
    Xt0 = torch.from_numpy(np.ascontiguousarray(start.T)).to(DEV)
    a = Xt0.clone()
    res = ST.stein_variational_refine_t(a, _gaussian_score_t, blocks, 4, EPS, scale=scale, circular=WRAP3)
    assert res["steps"] == 4 and tuple(res["hist"].shape) == (3, 65) and list(res["cols"]) == list(flat)
    m = Xt0.clone()
    table = nh.pack_mmd_blocks([2, 1], np.sqrt([2.0, 1.0]))
    hist = torch.zeros(3, 65, dtype=torch.float64, device=DEV)
    for t in range(4):
        Phi = nh.svgd_direction_t(m, _gaussian_score_t(m), table, flat, scale=scale[flat], wrap=WRAP3[flat])
        nh.sample_step_t(m, flat, Phi, hist, np.full(3, EPS), wrap=WRAP3[flat], first=t == 0)
    assert torch.equal(a, m) and torch.equal(res["hist"], hist) and not torch.equal(a, Xt0)
    b = Xt0.clone()
    again = ST.stein_variational_refine_t(b, _gaussian_score_t, blocks, 4, EPS, scale=scale, circular=WRAP3)
    assert torch.equal(a, b) and torch.equal(res["hist"], again["hist"])
    z = Xt0.clone()
    none = ST.stein_variational_refine_t(z, _gaussian_score_t, blocks, 0, EPS, scale=scale, circular=WRAP3)
    assert none["steps"] == 0 and torch.equal(z, Xt0)
    # the row-major convenience form, the score a callable on numpy
    from test_sample_svgd_cpu import gaussian_score
    row = ST.stein_variational_refine(start, gaussian_score, blocks, 4, EPS, scale=scale, circular=WRAP3, device=DEV)
    assert row["x"].dtype == np.float32 and row["x"].shape == (65, 3) and row["steps"] == 4
    assert np.max(np.abs(row["x"].astype(np.float64) - _host(a).T) / np.abs(_host(a).T)) <= 2.0 ** -22


@pytest.mark.parametrize("n", (65, 130))
@pytest.mark.parametrize("split", (False, True))
def test_device_meets_the_svgd_conditions(n, split):
    start, scale = gaussian_case(n)
    Xt = torch.from_numpy(np.ascontiguousarray(start.T)).to(DEV)
    ST.stein_variational_refine_t(Xt, _gaussian_score_t, gaussian_blocks(split), 500, EPS, scale=scale, circular=WRAP3)
    assert_svgd_conditions(_host(Xt).T, "device, n = %d, %s" % (n, "blocks {0, 1}, {2}" if split else "one joint block"))


def test_device_meets_the_ascent_condition():
    start, scale = gaussian_case(65)
    Xt = torch.from_numpy(np.ascontiguousarray(start.T)).to(DEV)
    ST.stein_variational_refine_t(Xt, _gaussian_score_t, [[0, 1, 2]], 300, EPS, circular=WRAP3, kernel=False)
    assert_ascent_condition(_host(Xt).T, "device ascent")


# ---- 5. the C entries ----------------------------------------------------------------------------------------------------------------
def test_c_entry_refusals_and_nan_for_a_bad_block_only():
    n, rows = 8, 4
    X = torch.zeros(rows, n, dtype=torch.float32, device=DEV)
    G = torch.ones(rows, n, dtype=torch.float64, device=DEV)
    table = nh.pack_mmd_blocks([2, 1], [1.0, 1.0])
    tdev, cols = nh.upload(table.view(np.uint8).reshape(-1), np.array([0, 1, 3], dtype=np.int32), device=DEV)
    phi = torch.zeros(3, n, dtype=torch.float64, device=DEV)
    scr = torch.zeros(int(nh.lib().nfisam_sample_svgd_scratch_count(n, 2, 3)), dtype=torch.float64, device=DEV)
    assert scr.numel() == 3 * 64
    call, null = nh.lib().nfisam_sample_svgd, C.c_void_p(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    host = lambda t: t.ctypes.data_as(C.c_void_p)
    ok = (ptr(X), rows, n, ptr(G), host(table), ptr(tdev), 2, ptr(cols), 3, null, null, ptr(phi), ptr(scr), null)

    def bad_table(field, value, b=1):
        t = table.copy()
        t[field][b] = value
        return t

    tables = [bad_table("d", 0), bad_table("inv_two_sigma2", 0.0), bad_table("inv_two_sigma2", -1.0),
              bad_table("inv_two_sigma2", np.inf), bad_table("inv_two_sigma2", np.nan), bad_table("col_off", 1)]
    for k, bad in [(0, null), (3, null), (4, null), (5, null), (7, null), (11, null), (12, null), (1, 0), (2, 0), (6, 0), (8, 0),
                   (2, 65535 * 64 + 1), (6, 65536)] + [(4, host(t)) for t in tables]:
        args = list(ok)
        args[k] = bad
        assert call(*args) == nh.ERR_ARG, k
    assert call(*ok) == nh.OK
    torch.cuda.synchronize()
    assert np.array_equal(_host(phi), np.ones((3, n)))                 # all points coincide: k = 1, d = 0, phi = the mean score

    # a row outside the matrix in the DEVICE list, a block that leaves the entries in the DEVICE table: NaN for that block only
    bad_cols, = nh.upload(np.array([0, 1, rows], dtype=np.int32), device=DEV)
    args = list(ok)
    args[7] = ptr(bad_cols)
    phi.zero_()
    assert call(*args) == nh.OK
    torch.cuda.synchronize()
    assert np.array_equal(_host(phi)[:2], np.ones((2, n))) and np.all(np.isnan(_host(phi)[2]))
    bad_dev, = nh.upload(bad_table("d", 2).view(np.uint8).reshape(-1), device=DEV)                   # entries 2 .. 4 of 3
    args = list(ok)
    args[5] = ptr(bad_dev)
    phi.zero_()
    assert call(*args) == nh.OK
    torch.cuda.synchronize()
    assert np.array_equal(_host(phi)[:2], np.ones((2, n))) and np.all(np.isnan(_host(phi)[2]))

    hist = torch.zeros(3, n, dtype=torch.float64, device=DEV)
    eps, = nh.upload(np.full(3, 0.5), device=DEV)
    phi.fill_(2.0)
    scall = nh.lib().nfisam_sample_step
    dbl = C.c_double
    sok = (ptr(X), rows, n, ptr(cols), 3, null, ptr(phi), ptr(hist), ptr(eps), dbl(0.9), dbl(1e-6), 1, null)
    for k, bad in ((0, null), (3, null), (6, null), (7, null), (8, null), (1, 0), (2, 0), (4, 0), (4, 65536), (9, dbl(1.0)),
                   (9, dbl(-0.1)), (9, dbl(np.nan)), (10, dbl(0.0)), (10, dbl(-1.0)), (10, dbl(np.inf)), (10, dbl(np.nan))):
        args = list(sok)
        args[k] = bad
        assert scall(*args) == nh.ERR_ARG, k
    assert scall(*sok) == nh.OK
    torch.cuda.synchronize()
    want = np.zeros((rows, n), dtype=np.float32)
    want[[0, 1, 3]] = np.float32(0.5 * 2.0 / (2.0 + 1e-6))
    assert np.array_equal(_host(X), want) and np.array_equal(_host(hist), np.full((3, n), 4.0))
    args = list(sok)
    args[3] = ptr(bad_cols)                                            # no such row: nothing moves, NaN in its hist
    assert scall(*args) == nh.OK
    torch.cuda.synchronize()
    assert np.array_equal(_host(X)[2], np.zeros(n)) and np.all(np.isnan(_host(hist)[2])) and np.all(np.isfinite(_host(hist)[:2]))


def test_bindings_refuse_wrong_tensors_on_the_device():
    Xt = torch.zeros(3, 5, dtype=torch.float32, device=DEV)
    Gt = torch.zeros(3, 5, dtype=torch.float64, device=DEV)
    t = nh.pack_mmd_blocks([3], [1.0])
    with pytest.raises(ValueError, match="contiguous float64"):
        nh.svgd_direction_t(Xt, Gt.float(), t, [0, 1, 2])
    with pytest.raises(ValueError, match="contiguous float32"):
        nh.svgd_direction_t(Xt.double(), Gt, t, [0, 1, 2])
    with pytest.raises(ValueError, match="shape of the points"):
        nh.svgd_direction_t(Xt, Gt[:2].contiguous(), t, [0, 1, 2])
    with pytest.raises(ValueError, match="contiguous float64"):
        nh.svgd_direction_t(Xt, torch.zeros(5, 3, dtype=torch.float64, device=DEV).t(), t, [0, 1, 2])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.svgd_direction_t(Xt, Gt.cpu(), t, [0, 1, 2])
    with pytest.raises(ValueError, match=r"Phi must be \[n_entries, n\]"):
        nh.sample_step_t(Xt, [0, 1], Gt, Gt.clone(), np.ones(2))
    with pytest.raises(ValueError, match="named more than once"):
        nh.sample_step_t(Xt, [0, 1, 1], Gt, Gt.clone(), np.ones(3))
    with pytest.raises(ValueError, match="eps must have one value per entry"):
        nh.sample_step_t(Xt, [0, 1, 2], Gt, Gt.clone(), np.ones(2))
    with pytest.raises(ValueError, match="alpha"):
        nh.sample_step_t(Xt, [0, 1, 2], Gt, Gt.clone(), np.ones(3), alpha=1.0)
    assert torch.equal(Xt, torch.zeros_like(Xt))


# ---- 6. the solver --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_range(tmp_path_factory):
    """The small range problem through its six updates, once for the tests below: (solver, the last update's samples,
    arguments): the recipe of tests/test_sample_ksd_gpu.py, trained with the fixture's own arguments, unchanged."""
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
    fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
    kwargs = json.loads(str(fx["arguments"]))
    kwargs["cuda_training"] = True
    path = tmp_path_factory.mktemp("small_range") / "factor_graph.fg"
    path.write_text(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    nodes, truth, factors = graph_file_parser(str(path), "fg", prior_cov_scale=0.1)
    steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))
    solver = NFiSAM(NFiSAMArgs(**kwargs))
    for vs, fs in steps:
        for v in vs: solver.add_node(v)
        for f in fs: solver.add_factor(f)
        solver.update_physical_and_working_graphs()
        smp = solver.incremental_inference()
    return solver, {v: np.array(smp[v]) for v in solver.elimination_ordering}, kwargs


def test_small_range_posterior_refine(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    n = len(smp[order[0]])
    log_p = solver.joint_log_pdf(smp)
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
             list(order), len(solver.physical_factors))
    for kernel in ("variable", "joint", None):
        out = solver.posterior_refine(smp, steps=3, kernel=kernel)
        assert set(out) == {"samples", "log_p_before", "log_p_after", "steps", "kernel", "sigma", "precision", "n"}
        assert out["n"] == n and out["steps"] == 3 and out["kernel"] == kernel and set(out["samples"]) == set(order)
        for v in order:
            a = out["samples"][v]
            assert a.shape == (n, v.dim) and a.dtype == np.float32 and np.all(np.isfinite(a))
            assert out["precision"][v].shape == (v.dim,) and np.all(out["precision"][v] >= 0)
        assert any(not np.array_equal(out["samples"][v], smp[v].astype(np.float32)) for v in order)
        assert out["log_p_before"].dtype == np.float64 and np.array_equal(out["log_p_before"], log_p)
        assert out["log_p_after"].shape == (n,) and np.all(np.isfinite(out["log_p_after"]))
        again = solver.posterior_refine(smp, steps=3, kernel=kernel)
        assert all(np.array_equal(again["samples"][v], out["samples"][v]) for v in order)
        assert np.array_equal(again["log_p_after"], out["log_p_after"])
        # valid input to the other evaluations
        assert np.array_equal(solver.joint_log_pdf(out["samples"]), out["log_p_after"])
        assert np.isfinite(solver.posterior_ksd(out["samples"])["vstat"])
        print("kernel = %r, 3 steps: mean log p %.6f -> %.6f" % (kernel, log_p.mean(), out["log_p_after"].mean()))
    assert isinstance(solver.posterior_refine(smp, steps=1, kernel="joint")["sigma"], float)
    assert set(solver.posterior_refine(smp, steps=1)["sigma"]) == set(order)
    zero = solver.posterior_refine(smp, steps=0)
    assert zero["steps"] == 0 and np.array_equal(zero["log_p_after"], zero["log_p_before"])
    assert all(np.array_equal(zero["samples"][v], smp[v].astype(np.float32)) for v in order)
    # nothing of the solver's state or of the random streams was touched: a following draw is what it would have been
    assert torch.equal(state[0], torch.get_rng_state()) and torch.equal(state[1], torch.cuda.get_rng_state())
    assert np.array_equal(state[2], np.random.get_state()[1]) and state[3] == random.getstate()
    assert state[4] == list(solver.elimination_ordering) and state[5] == len(solver.physical_factors)
    own = solver.posterior_refine(n=257, steps=2)
    assert own["n"] == 257 and all(own["samples"][v].shape == (257, v.dim) for v in order)
    assert np.all(np.isfinite(own["log_p_after"]))
    for bad in (dict(steps=-1), dict(step_size=0.0), dict(step_size=[0.1, 0.1]), dict(kernel="block"), dict(sigma=-1.0),
                dict(kernel="joint", sigma=[1.0, 2.0])):
        with pytest.raises(ValueError, match="posterior_refine"):
            solver.posterior_refine(smp, **bad)
    with pytest.raises(ValueError, match="samples lack"):
        solver.posterior_refine({})


def test_small_range_map_refine(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    start = solver.joint_log_pdf(smp).max()
    out = solver.map_refine(smp, steps=20)
    assert set(out) == {"map_sample", "log_p", "start_log_p", "improved", "climbers", "steps", "top", "n"}
    assert out["start_log_p"] == start and out["log_p"] >= out["start_log_p"]
    assert out["improved"] == (out["log_p"] > out["start_log_p"]) and isinstance(out["improved"], bool)
    assert out["climbers"].shape == (8,) and out["climbers"].max() == out["log_p"] and out["top"] == 8
    assert all(out["map_sample"][v].shape == (v.dim,) for v in order)
    again = solver.joint_log_pdf({v: out["map_sample"][v][None, :] for v in order})
    assert again.shape == (1,) and again[0] == out["log_p"]
    best = solver.map_estimate(smp)
    assert solver.joint_log_pdf({v: np.asarray(best[v])[None, :] for v in order})[0] == out["start_log_p"]
    print("map_refine, 20 steps: log p %.6f -> %.6f (improved: %s)" % (out["start_log_p"], out["log_p"], out["improved"]))
    still = solver.map_refine(smp, steps=0, top=3)
    assert still["log_p"] == start and not still["improved"] and still["climbers"].shape == (3,)
    for bad in (dict(top=0), dict(top=1.5), dict(steps=-1), dict(step_size=np.inf)):
        with pytest.raises(ValueError, match="map_refine"):
            solver.map_refine(smp, **bad)
