"""The kernel Stein discrepancy on the GPU (nfisam_sample_ksd, nfisam_hip.ksd_sums, utils.Statistics, NFiSAM.posterior_ksd)
against the reference's own run stored in tests/golden/factor_score.npz part (c), against the float64 numpy restatement of
tests/test_sample_ksd_cpu.py across the tile and chunk boundaries, and its bitwise promises.

Bounds, |device - yardstick| <= TOL (|yardstick| + 1), each 16 x the largest deviation measured on the MI355X
(DEVICE_MEASURED below, recorded in profiles/ksd.json):
  * against the fixture: 1.4e-13 (row sums against off_ksd's row sums plus the diagonal: 1.36e-13; H against off_ksd 2.2e-14,
    diag 4.0e-16, ustats and vstats 0) -> 2.2e-12.  The host restatement's own deviation on the CPU is 5.1e-14
    (tests/test_sample_ksd_cpu.py): the device is within a factor of three of it;
  * against the restatement at n in {1, 2, 63, 64, 65, 130} x D in {1, 5, 16, 17, 33}, with and without wrapped columns and a
    zero-precision column: 1.8e-13 (n = 130) -> 2.9e-12.
p_u is compared exactly: the same multinomial draws, and no bootstrap value lies within rounding of ustats."""
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_factor_score_cpu import deviation, ksd_graph, score_fixture
from test_sample_ksd_cpu import bootstrap, stein_matrix, stein_stats
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEVICE_MEASURED = {"fixture": 1.4e-13, "numpy": 1.8e-13}
TOL = {k: 16 * v for k, v in DEVICE_MEASURED.items()}
KSD_SEED = 20261019                     # make_factor_score_fixture.py


def _host(sums):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in sums.items()}


def test_fixture_row_diag_matrix_statistics_and_bootstrap():
    fs = score_fixture()
    x, s, p = fs["ksd_samples"], fs["ksd_score"], fs["ksd_precision"]
    n = x.shape[0]
    out = nh.ksd_sums(x, s, p, matrix=True, device=DEV)
    assert all(out[k].dtype == torch.float64 for k in ("row", "diag", "H")) and tuple(out["H"].shape) == (n, n)
    got = _host(out)
    off = got["H"] - np.diag(np.diag(got["H"]))
    diag_ref = (s * s).sum(1) + p.sum()
    u, v = ST.ksd_from_sums(got["row"].sum(), got["diag"].sum(), n)
    d = dict(off=deviation(off, fs["ksd_off"]), diag=deviation(got["diag"], diag_ref),
             row=deviation(got["row"], fs["ksd_off"].sum(1) + diag_ref), ustats=deviation(u, fs["ksd_ustats"]),
             vstats=deviation(v, fs["ksd_vstats"]))
    print("fixture: |device - ref| / (|ref| + 1):", d)
    assert max(d.values()) <= TOL["fixture"], d
    assert np.array_equal(np.diag(got["H"]), got["diag"])
    boot = ST.ksd_bootstrap(out["H"], fs["ksd_draws"])
    assert deviation(boot, bootstrap(fs["ksd_off"], fs["ksd_draws"])) <= TOL["fixture"]
    assert float(np.mean(boot >= u)) == float(fs["ksd_p_u"])
    # the reference's name and return shape, the generator replayed from the fixture's seed; a diagonal matrix is accepted
    us, p_u, off2, vs = ST.Gaussian_kernel_stein_discrepancy(s, np.diag(p), x, nboot=fs["ksd_draws"].shape[0],
                                                             rng=np.random.RandomState(KSD_SEED), device=DEV)
    assert (us, vs) == (u, v) and p_u == float(fs["ksd_p_u"]) and np.array_equal(off2, off)

    class Joint:
        def grad_x_log_pdf(self, pts):
            assert pts.dtype == np.float64
            return s
    us3, p3, _, vs3 = ST.Gaussian_kernel_stein_discrepancy(Joint(), p, x, nboot=7, rng=np.random.RandomState(1), device=DEV)
    assert (us3, vs3) == (u, v) and 0.0 <= p3 <= 1.0
    # the same through the device score of the same graph
    variables, factors = ksd_graph(fs["ksd_truth"])
    col, o = {}, 0
    for var in variables:
        col[var] = o
        o += var.dim
    G = nh.factor_graph_score(nh.pack_factor_terms(factors, col), x, DEV)
    res = ST.kernel_stein_discrepancy(torch.from_numpy(x).to(DEV), G, sigma=1.0, scale=np.sqrt(p), nboot=20,
                                      rng=np.random.RandomState(3), matrix=True)
    assert np.allclose(res["precision"], p, rtol=1e-15, atol=0.0) and res["H"].shape == (n, n)
    # (the reference's SE(2) gradient is off by 7.5e-5 on these points: tests/test_factor_score_cpu.py)
    assert abs(res["ustat"] - u) <= 1e-3 * abs(u) and abs(res["vstat"] - v) <= 1e-3 * abs(v)
    assert res["row"].shape == (n,) and np.isclose(res["row"].sum() / n, res["vstat"], rtol=1e-13, atol=0.0)
    assert res["bootstrap"].shape == (20,) and 0.0 <= res["p_value"] <= 1.0


def _random_case(n, D, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, D) * rng.uniform(0.1, 3.0, D) + rng.uniform(-50, 50, D)).astype(np.float32)
    s = rng.randn(n, D) * rng.uniform(0.1, 30.0, D)
    p = rng.uniform(0.05, 2.0, D) / D
    return x, s, p


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 130))
def test_sums_match_the_numpy_restatement_across_tiles_and_chunks(n):
    worst = 0.0
    for D in (1, 5, 16, 17, 33):
        x, s, p = _random_case(n, D, 1000 * n + D)
        wrap = np.zeros(D, dtype=np.uint8)
        wrap[::3] = 1
        xw = x.copy()
        xw[:, wrap != 0] = np.random.RandomState(D).uniform(-3.1, 3.1, (n, int(wrap.sum()))).astype(np.float32)
        xw[0, 0] = 3.1
        if n > 1:
            xw[1, 0] = -3.1                                        # a pair across the seam: 0.083 rad apart, not 6.2
        pz = p.copy()
        pz[D // 2] = 0.0                                           # a column that leaves the kernel (its scores stay in s.s)
        for pts, prec, wr in ((x, p, None), (xw, p, wrap), (x, pz, None), (xw, pz, wrap)):
            got = _host(nh.ksd_sums(pts, s, prec, wrap=wr, matrix=True, device=DEV))
            H = stein_matrix(pts, s, prec, wr)
            d = max(deviation(got["H"], H), deviation(got["row"], H.sum(1)), deviation(got["diag"], np.diag(H)))
            worst = max(worst, d)
            assert np.array_equal(got["H"], got["H"].T)            # symmetric to the bit
            u, v = ST.ksd_from_sums(got["row"].sum(), got["diag"].sum(), n, ustat=n >= 2)
            u_ref, v_ref = stein_stats(H)
            assert deviation(v, v_ref) <= TOL["numpy"] and (n < 2 or deviation(u, u_ref) <= TOL["numpy"])
        if n > 1:
            assert stein_matrix(xw, s, p, wrap)[0, 1] != stein_matrix(xw, s, p)[0, 1]
    print("n = %3d: |device - numpy| / (|numpy| + 1) = %.3g" % (n, worst))
    assert worst <= TOL["numpy"], worst


def test_bits_with_and_without_the_matrix_and_on_a_second_call():
    x, s, p = _random_case(130, 17, 5)
    wrap = np.zeros(17, dtype=np.uint8)
    wrap[2] = 1
    a = _host(nh.ksd_sums(x, s, p, wrap=wrap, matrix=True, device=DEV))
    b = _host(nh.ksd_sums(x, s, p, wrap=wrap, matrix=False, device=DEV))
    c = _host(nh.ksd_sums(torch.from_numpy(x).to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(p).to(DEV), wrap=wrap,
                          matrix=True))
    assert b["H"] is None
    assert np.array_equal(a["row"], b["row"]) and np.array_equal(a["diag"], b["diag"])
    assert all(np.array_equal(a[k], c[k]) for k in ("row", "diag", "H"))
    assert np.array_equal(a["H"], a["H"].T)
    # the column-major entry on the matrices in place
    Xt = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    Gt = torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV)
    t = _host(nh.ksd_sums_t(Xt, Gt, p, wrap=wrap))
    assert np.array_equal(t["row"], a["row"]) and np.array_equal(t["diag"], a["diag"])


def test_c_entry_refusals():
    import ctypes as C
    X = torch.zeros(2, 8, dtype=torch.float32, device=DEV)
    G = torch.zeros(2, 8, dtype=torch.float64, device=DEV)
    p = torch.ones(2, dtype=torch.float64, device=DEV)
    row, diag = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    scr = torch.zeros(64, dtype=torch.float64, device=DEV)
    call, null = nh.lib().nfisam_sample_ksd, C.c_void_p(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ok = (ptr(X), ptr(G), 2, 8, ptr(p), null, ptr(row), ptr(diag), null, ptr(scr), null)
    for k, bad in ((0, null), (1, null), (4, null), (6, null), (7, null), (9, null), (2, 0), (3, 0), (3, 65535 * 64 + 1)):
        args = list(ok)
        args[k] = bad
        assert call(*args) == nh.ERR_ARG, k
    args = list(ok)
    args[3], args[8] = 4097, ptr(scr)                               # the matrix for more than 4096 points
    assert call(*args) == nh.ERR_ARG
    assert call(*ok) == nh.OK
    torch.cuda.synchronize()
    assert np.array_equal(row.cpu().numpy(), np.full(8, 16.0)) and np.array_equal(diag.cpu().numpy(), np.full(8, 2.0))


@pytest.fixture(scope="module")
def small_range(tmp_path_factory):
    """The small range problem through its six updates, once for the tests below: (solver, the last update's samples,
    arguments).  Trained with the fixture's own arguments, unchanged -- the reference's run script's budget, 2000 iterations
    with the window early stop (under a second here): no budget of this file's own choosing
    (other tests cut it to 200 .. 300 iterations for speed; see the ordering test below on what that does to it)."""
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


def test_small_range_pipeline_posterior_ksd(small_range):
    """`posterior_ksd()` runs and returns finite numbers, `joint_score` is `factor_graph_score` of the same points, and a
    repeated call gives the same values."""
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    n = len(smp[order[0]])
    pcol, total = solver._post_columns()
    S = np.zeros((n, total), dtype=np.float32)
    for v in order:
        S[:, pcol[v]:pcol[v] + v.dim] = smp[v]
    G = solver.joint_score(smp)
    assert G.shape == (n, total) and G.dtype == np.float64 and np.all(np.isfinite(G))
    assert np.array_equal(G, nh.factor_graph_score(nh.pack_factor_terms(solver.physical_factors, pcol), S, DEV).cpu().numpy())
    base = solver.posterior_ksd(smp, nboot=25, seed=11)
    assert base["n"] == n and np.isfinite(base["ustat"]) and np.isfinite(base["vstat"]) and 0.0 <= base["p_value"] <= 1.0
    assert base["row_mean"].shape == (n,) and np.all(np.isfinite(base["row_mean"])) and base["bootstrap"].shape == (25,)
    assert set(base["precision"]) == set(order) and all(np.all(p >= 0) for p in base["precision"].values())
    again = solver.posterior_ksd(smp, nboot=25, seed=11)
    assert again["ustat"] == base["ustat"] and again["vstat"] == base["vstat"] and again["p_value"] == base["p_value"]
    # its own draw through the tree walk, where the matrix lies
    own = solver.posterior_ksd(n=257)
    assert own["n"] == 257 and np.isfinite(own["ustat"]) and np.isfinite(own["vstat"])
    assert len(solver.posterior_ksd()["row_mean"]) == kwargs["posterior_sample_num"]
    raw = solver.posterior_ksd(smp, standardise=False, sigma=2.0)
    assert np.isfinite(raw["vstat"]) and all(np.all(p == 0.25) for p in raw["precision"].values())


def test_small_range_posterior_beats_the_same_draw_with_its_landmarks_moved(small_range):
    """The sanity ordering the feature was specified with: the V-statistic of the trained posterior's draw is smaller than
    that of the same draw with every landmark column moved by three of its standard deviations.

    Measured on the MI355X, at the reference's own budget (the fixture's arguments: 2000 iterations, window early stop):
        V  posterior draw 469652.82   landmarks + 3 std 469661.52        U  459298.57 / 459307.26
    The margin is small and the training budget matters.  With the budget cut to 300 iterations the ordering does NOT hold:
        V  posterior draw 626923.37   landmarks + 3 std 626917.76   (+ 1 std 626915.44, + 10 std 627040.03)
    The cause is in the posterior, not in the sums (which agree with the numpy restatement and the reference's run to
    2e-13): the statistic is in the units of the score, and the heading columns of X1 .. X4 carry scores of rms 1e3 (a
    heading moves the next pose sideways by 30 m against an odometry sigma of 0.04 m) whose MEANS over an under-trained
    posterior are -510 .. +900, the pose xy columns means of up to 30, while a landmark's score is of order 1 (range sigma
    2 m).  Moving the landmarks changes V by the positive quadratic term mean(k) |delta s|^2 (about +80) and by the cross
    term 2 mean(k s_pose) . delta s_pose through the range factors' pose ends, which has either sign and the size of the
    pose score means times |delta s| (about -85 at 300 iterations).  The heading score means are no smaller at the full budget
    (-902 .. +468): there the cross term happens to be the smaller one.  The ordering is a property of this run, tested as
    specified, not something the statistic guarantees for a posterior this far from p in its stiffest columns."""
    from slam.Variables import VariableType
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    base = solver.posterior_ksd(smp)
    shifted = {v: smp[v].astype(np.float64) + (3.0 * smp[v].astype(np.float64).std(0) if v.type == VariableType.Landmark else 0.0)
               for v in order}
    moved = solver.posterior_ksd(shifted)
    print("V-statistic: posterior draw %.8g, landmarks moved by three standard deviations %.8g" % (base["vstat"], moved["vstat"]))
    assert np.isfinite(base["vstat"]) and np.isfinite(moved["vstat"])
    assert base["vstat"] < moved["vstat"]
