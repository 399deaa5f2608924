"""The two-sample MMD on the GPU (nfisam_sample_mmd through nfisam_hip.mmd_sums, utils.Statistics.mmd_blocks and
NFiSAM.posterior_mmd).

The oracle of the kernel sums is a float64 numpy evaluation by direct differences, broadcast as (m, n, d), at the same
float32 points (`oracle_sums` of tests/test_sample_mmd_cpu.py).  Bound: |S_dev - S_ref| <= 1e-11 S_ref + 1e-300.  Every term
is positive, so a sum's relative error is at most the largest term's plus the accumulation's; a term exp(a) has relative
error at most about |a| (d + 2) 2^-53 plus the exp itself: with |a| <= 745 and d <= 40 under 4e-12.

The 5 m shift of the solver test: MMDb^2 = floor^2 + (sum of k over DISTINCT pairs of x) / m^2 + (the same of y) / n^2
- 2 Sxy / mn, so MMDb sits at floor = sqrt(1 / m + 1 / n) exactly when no two distinct points -- of the two sets or of one
-- are within kernel reach.  A posterior draw's own points are within reach of each other at any bandwidth of its own
scale, so that test standardises the columns (unit spread) and uses sigma = 0.002: MMDb leaves floor by more than 1e-6 only
if the k of distinct pairs add up to 0.03 (m = n = 500), i.e. if some pair is closer than 2.6 sigma = 0.005 spreads; among
the 125000 pairs of 500 points that fill even only three effective dimensions about 125000 (0.005 / 2.5)^3 = 0.001 are, and
float32 resolves 1e-5 spreads.  The shifted set is at least 2.5 spreads away in every column.  At the default bandwidth the
same shifted reference must read far above floor where the posterior is narrow: the first pose, pinned by its prior to
well under 1 m, has E k(x, x') > 1 / 2 at sigma^2 = 2 and k < exp(-50 / 4) across, so its MMDb exceeds 1."""
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_mmd_cpu import oracle_sums
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
RTOL, ATOL = 1e-11, 1e-300
M_MAX, N_MAX, COLS = 130, 200, 64


def _data():
    """x [130, 64], y [200, 64] float32: columns 0..55 Gaussian around 3 (spread 1.5 / 1.2), 56..58 a pose block whose third
    column is a heading spread over the whole circle, 60..61 two sets 18 apart."""
    rng = np.random.RandomState(11)
    x = rng.standard_normal((M_MAX, COLS)) * 1.5 + 3.0
    y = rng.standard_normal((N_MAX, COLS)) * 1.2 + 3.3
    x[:, 58] = rng.uniform(-np.pi, np.pi, M_MAX)
    y[:, 58] = rng.uniform(-np.pi, np.pi, N_MAX)
    x[:, 60:62] = rng.standard_normal((M_MAX, 2))
    y[:, 60:62] = rng.standard_normal((N_MAX, 2)) + 18.0
    return x.astype(np.float32), y.astype(np.float32)


def _table():
    """The 14 blocks: (xcols, ycols, sigma, scale or None, wrap or None)."""
    rng = np.random.RandomState(12)
    r = lambda a, b: list(range(a, b))                                                        # noqa: E731
    sq = lambda d: float(np.sqrt(d))                                                          # noqa: E731
    return [
        ([0], [0], sq(1), None, None), ([1], [1], sq(1), None, None),                         # d = 1, contiguous
        ([5, 37], [5, 37], sq(2), None, None), ([0, 1], [0, 1], sq(2), None, None),           # scattered; over the d = 1 blocks
        ([2, 3, 2], [2, 3, 2], sq(3), None, None), ([6, 7, 8], [6, 7, 8], 1.0, None, None),   # a repeated column; sigma fixed
        (r(10, 26), r(10, 26), sq(16), None, None), (r(20, 36), r(20, 36), sq(16), None, None),
        (r(10, 27), r(10, 27), sq(17), None, None), (r(30, 47), list(range(46, 29, -1)), sq(17), None, None),   # xcols != ycols
        (r(0, 40), r(0, 40), sq(40), None, None), (r(8, 48), r(8, 48), sq(40), list(rng.uniform(0.5, 2.0, 40)), None),
        ([60, 61], [60, 61], 0.7, None, None),                                                # far apart: exponents from ~400 to past exp's range
        ([56, 57, 58], [56, 57, 58], 0.5, None, [0, 0, 1]),                                   # a pose with its heading
    ]


def _arrays(table):
    dims = [len(b[0]) for b in table]
    blocks = nh.pack_mmd_blocks(dims, [b[2] for b in table])
    xcols = np.concatenate([b[0] for b in table]).astype(np.int32)
    ycols = np.concatenate([b[1] for b in table]).astype(np.int32)
    scale = np.concatenate([np.ones(len(b[0])) if b[3] is None else np.asarray(b[3], dtype=np.float64) for b in table]) \
        if any(b[3] is not None for b in table) else None
    wrap = np.concatenate([np.zeros(len(b[0]), dtype=np.uint8) if b[4] is None else np.asarray(b[4], dtype=np.uint8)
                           for b in table]) if any(b[4] is not None for b in table) else None
    return blocks, xcols, ycols, scale, wrap


def _oracle(x, y, table):
    return np.stack([oracle_sums(x, y, b[0], b[1], 1.0 / (2.0 * b[2] ** 2), b[3], b[4]) for b in table])


def _excess(dev, ref):
    """max |dev - ref| / (RTOL ref + ATOL): <= 1 inside the bound."""
    return float(np.max(np.abs(dev - ref) / (RTOL * ref + ATOL)))


@pytest.mark.parametrize("n", [1, 64, 200])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_sums_match_the_float64_oracle(m, n):
    """All 14 blocks in one table at every (m, n) around the 64-point tile.  Largest |dev - ref| / ref measured on the MI355X
    over all 15 cases: 4.2e-16 (6.1e-16 over the 783 blocks of the final Plaza1 tree at n = 500, 8.1e-16 at n = 2000:
    profiles/r10_sample_mmd.json, `max_rel_dev`); the bound stays the 1e-11 of the error analysis."""
    x, y = _data()
    x, y = x[:m], y[:n]
    table = _table()
    blocks, xcols, ycols, scale, wrap = _arrays(table)
    dev = nh.mmd_sums(x, y, blocks, xcols, ycols, scale, wrap, device=DEV).cpu().numpy()
    ref = _oracle(x, y, table)
    assert dev.shape == (14, 3) and dev.dtype == np.float64
    rel = np.abs(dev - ref) / np.maximum(ref, 1e-300)
    print("m %d n %d: largest relative deviation %.3g (block %d)" % (m, n, rel.max(), int(np.argmax(rel.max(1)))))
    assert np.all(np.isfinite(dev)) and _excess(dev, ref) <= 1.0, (dev, ref)
    assert np.all(dev[:, 0] >= m) and np.all(dev[:, 1] >= n)                 # each i = i pair contributes exactly 1
    if m == 1:
        assert np.all(dev[:, 0] == 1.0)
    if n == 1:
        assert np.all(dev[:, 1] == 1.0)


def test_chunk_boundary_widths_at_a_tile_boundary():
    """Blocks of 16, 17 and 33 columns -- one staged chunk of 16, a chunk plus one column, two chunks plus one -- at
    m = n = 65, one point past the 64-point tile on both sides; with a scale and a wrapped column, and without.  The 14-block
    table above reaches widths 16, 17 and 40 but not 33, and n = 65 on the x side only."""
    x, y = _data()
    x, y = x[:65], y[:65]
    r = lambda a, b: list(range(a, b))                                                        # noqa: E731
    rng = np.random.RandomState(13)
    plain = [(r(a, a + d), r(a, a + d), float(np.sqrt(d)), None, None) for a, d in ((3, 16), (20, 17), (7, 33))]
    wrapped = [(r(26, 59), r(26, 59), float(np.sqrt(33)), list(rng.uniform(0.5, 2.0, 33)), [0] * 32 + [1])]     # 58: the heading
    for table in (plain, plain + wrapped):
        dev = nh.mmd_sums(x, y, *_arrays(table), device=DEV).cpu().numpy()
        ref = _oracle(x, y, table)
        print("widths %s: largest relative deviation %.3g" % ([len(b[0]) for b in table], (np.abs(dev - ref) / ref).max()))
        assert np.all(np.isfinite(dev)) and _excess(dev, ref) <= 1.0, (dev, ref)


def test_second_call_single_blocks_and_reversed_table_give_the_same_bits():
    x, y = _data()
    x, y = x[:M_MAX], y[:N_MAX]
    table = _table()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    first = nh.mmd_sums(xd, yd, *_arrays(table)).cpu().numpy()
    again = nh.mmd_sums(xd, yd, *_arrays(table)).cpu().numpy()
    assert np.array_equal(first, again)
    rev = nh.mmd_sums(xd, yd, *_arrays(table[::-1])).cpu().numpy()
    assert np.array_equal(rev[::-1], first)
    for k, b in enumerate(table):                        # alone (and without scale / wrap arrays where the block has none)
        alone = nh.mmd_sums(xd, yd, *_arrays([b])).cpu().numpy()
        assert np.array_equal(alone[0], first[k]), (k, alone, first[k])
    # the column-major twin uses the matrices in place and gives the same bits
    twin = nh.mmd_sums_t(xd.t().contiguous(), yd.t().contiguous(), *_arrays(table)).cpu().numpy()
    assert np.array_equal(twin, first)


def test_wrapped_headings():
    """Angles at +-3.13 are 0.023 rad apart on the circle and 6.26 apart on the line: MMDb = sqrt(2 (1 - k)) is 0.046 with
    k = exp(-2 * 0.0232^2) and sqrt(2) with k = exp(-2 * 6.26^2)."""
    rng = np.random.RandomState(3)
    x = (3.13 + 1e-3 * rng.standard_normal((70, 1))).astype(np.float32)
    y = (-3.13 + 1e-3 * rng.standard_normal((90, 1))).astype(np.float32)
    blocks = nh.pack_mmd_blocks([1], [0.5])
    on = nh.mmd_sums(x, y, blocks, [0], [0], wrap=np.ones(1, dtype=np.uint8), device=DEV).cpu().numpy()
    off = nh.mmd_sums(x, y, blocks, [0], [0], device=DEV).cpu().numpy()
    ref_on = oracle_sums(x, y, [0], [0], 2.0, wrap=[1])
    ref_off = oracle_sums(x, y, [0], [0], 2.0)
    assert _excess(on[0], ref_on) <= 1.0 and _excess(off[0], ref_off) <= 1.0
    assert on[0, 2] / (70 * 90) > 0.998 and off[0, 2] / (70 * 90) < 1e-30       # k ~ exp(-2 * 0.0232^2) vs exp(-2 * 6.26^2)
    assert off[0, 2] > 0.0
    got = ST.mmd_blocks(x, y, [[0]], sigma=0.5, circular=[True], device=DEV)
    assert got[0] < 0.1 and ST.mmd_blocks(x, y, [[0]], sigma=0.5, device=DEV)[0] > 1.3


def test_limits_far_sets_sit_at_floor_and_a_set_against_itself_at_zero():
    i, j = np.arange(64, dtype=np.float32), np.arange(70, dtype=np.float32)
    x = np.stack([100.0 * i, np.zeros_like(i)], 1)
    y = np.stack([100.0 * j, np.full_like(j, 1000.0)], 1)                      # 1e3 apart, every point 100 from its neighbours
    sums = nh.mmd_sums(x, y, nh.pack_mmd_blocks([2], [1.0]), [0, 1], [0, 1], device=DEV).cpu().numpy()
    assert sums[0, 2] == 0.0 and sums[0, 0] == 64.0 and sums[0, 1] == 70.0
    floor = np.sqrt(1.0 / 64 + 1.0 / 70)
    assert abs(ST.mmd_blocks(x, y, [[0, 1]], sigma=1.0, device=DEV)[0] - floor) <= 1e-15
    xs, _ = _data()
    same = ST.mmd_blocks(xs, xs, [[0, 1], list(range(10, 27)), list(range(0, 40))], device=DEV)
    print("MMDb of a set against itself:", same)
    assert np.all(same <= 1e-7)


def test_a_bad_block_given_to_the_c_entry_yields_nan_and_leaves_the_others_alone():
    """`checked=True` skips the binding's table check: the C entry sees a row past x_rows and a block past n_entries."""
    x, y = _data()
    table = _table()[:6]
    blocks, xcols, ycols, _, _ = _arrays(table)
    good = nh.mmd_sums(x, y, blocks, xcols, ycols, device=DEV).cpu().numpy()
    Xt, Yt = torch.from_numpy(x.T.copy()).to(DEV), torch.from_numpy(y.T.copy()).to(DEV)
    bad_x = xcols.copy()
    bad_x[3] = COLS                                      # block 2 = entries 2..3: one row past the matrix
    got = nh.mmd_sums_t(Xt, Yt, blocks, bad_x, ycols, checked=True).cpu().numpy()
    assert np.all(np.isnan(got[2, [0, 2]])) and got[2, 1] == good[2, 1]         # Syy reads ycols alone
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(got[keep], good[keep])
    bad_y = ycols.copy()
    bad_y[0] = -1
    got = nh.mmd_sums_t(Xt, Yt, blocks, xcols, bad_y, checked=True).cpu().numpy()
    assert np.all(np.isnan(got[0, [1, 2]])) and got[0, 0] == good[0, 0] and np.array_equal(got[1:], good[1:])
    past = blocks.copy()
    past["col_off"][5] = int(xcols.size) - 2             # d = 3: runs one entry past the lists
    got = nh.mmd_sums_t(Xt, Yt, past, xcols, ycols, checked=True).cpu().numpy()
    assert np.all(np.isnan(got[5])) and np.array_equal(got[:5], good[:5])
    with pytest.raises(ValueError):                                             # the binding's own check refuses all three
        nh.mmd_sums_t(Xt, Yt, past, xcols, ycols)
    with pytest.raises(ValueError):
        nh.mmd_sums_t(Xt, Yt, blocks, bad_x, ycols)


# ---- pinned to the reference --------------------------------------------------------------------------------------------------
def _xy_reorder(order, arr, ref_order):
    """icra_paper/compute_mmd.py:72-95 (`reorder_samples`): the xy columns of every variable, in `ref_order`."""
    off, col = 0, {}
    for v in order:
        col[v] = arr[:, off:off + 2]
        off += 3 if v.startswith("X") else 2
    return np.hstack([col[v] for v in ref_order])


def test_held_icra_results_of_the_reference():
    """Held run batches 1..3 against held reference steps 0..2, xy columns in the reference ordering: the device `mmd` and the
    per-variable marginal mean equal utils.Statistics.mmd on the same arrays; at step 0 (500 against 500: the reference's
    script downsamples nothing away) they are the values the reference published."""
    fx = np.load(os.path.join(GOLDEN, "pipeline_icra.npz"))
    for i in range(3):
        order = [str(v) for v in fx["held_run1_batch%d_ordering" % (i + 1)]]
        ref_order = [str(v) for v in fx["held_reference_step%d_ordering" % i]]
        run = _xy_reorder(order, fx["held_run1_batch%d" % (i + 1)], ref_order)
        ref = _xy_reorder(ref_order, fx["held_reference_step%d" % i], ref_order)
        nv = len(ref_order)
        got = ST.mmd_blocks(run, ref, [list(range(2 * nv))] + [[2 * k, 2 * k + 1] for k in range(nv)], estimator="mmd", device=DEV)
        r64, f64 = run.astype(np.float64), ref.astype(np.float64)
        want = np.array([ST.mmd(r64, f64)[0]] + [ST.mmd(r64[:, 2 * k:2 * k + 2], f64[:, 2 * k:2 * k + 2])[0] for k in range(nv)])
        print("step", i, "device", got, "numpy", want)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, equal_nan=True)
        np.testing.assert_allclose(np.mean(got[1:]), np.mean(want[1:]), rtol=1e-9, equal_nan=True)
        if i == 0:
            assert run.shape[0] == 500 and ref.shape[0] == 500
            assert abs(got[0] - float(fx["held_run1_mmd"][0])) <= 1e-7 and abs(got[0] - 0.01487791) <= 1e-7
            assert abs(np.mean(got[1:]) - float(fx["held_run1_marginal_mmd"][0])) <= 1e-7
            assert abs(np.mean(got[1:]) - 0.02299598) <= 1e-7


def test_values_of_the_reference_functions():
    """tests/golden/sample_mmd.npz: the reference's own MMDb and MMDu2 (make_sample_mmd_fixture.py)."""
    fx = np.load(os.path.join(GOLDEN, "sample_mmd.npz"))
    assert len(fx["cases"]) == 6
    for k, (m, n, d, sigma) in enumerate(fx["cases"]):
        x, y = fx["x%d" % k], fx["y%d" % k]
        assert x.shape == (int(m), int(d)) and y.shape == (int(n), int(d)) and x.dtype == np.float32
        cols = [list(range(int(d)))]
        b = ST.mmd_blocks(x, y, cols, estimator="MMDb", sigma=sigma, device=DEV)[0]
        u = ST.mmd_blocks(x, y, cols, estimator="MMDu2", sigma=sigma, device=DEV)[0]
        assert np.isclose(b, float(fx["MMDb%d" % k]), rtol=1e-9, atol=0), (k, b, float(fx["MMDb%d" % k]))
        assert np.isclose(u, float(fx["MMDu2%d" % k]), rtol=1e-9, atol=0), (k, u, float(fx["MMDu2%d" % k]))


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def test_posterior_mmd_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem, then: a second draw of the solver's own posterior is closer than floor in
    every marginal; a draw shifted by 5 m sits at floor where nothing is within reach (module docstring) and far above it at
    the default bandwidth; scoring the device draw in place equals scoring the same points handed over; a variable's
    marginal is `mmd_blocks` on that variable's columns."""
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
    first = {v: np.array(a) for v, a in solver.sample_posterior().items()}
    second = {v: np.array(a) for v, a in solver.sample_posterior().items()}
    n = len(first[order[0]])

    own = solver.posterior_mmd(second, first)
    assert own["m"] == n and own["n"] == n and own["estimator"] == "mmd" and own["floor"] == np.sqrt(2.0 / n)
    assert set(own["marginal"]) == set(order) and own["blocks"] == []
    marg = {v.name: (0.0 if np.isnan(a) else a) for v, a in own["marginal"].items()}     # NaN: closer than the estimator's noise
    print("own second draw:", own["joint"], marg, "floor", own["floor"])
    assert all(a < own["floor"] for a in marg.values()), (marg, own["floor"])

    shifted = {v: a + np.array([5.0, 5.0] + [0.0] * (v.dim - 2)) for v, a in second.items()}
    sat = solver.posterior_mmd(shifted, first, estimator="MMDb", sigma=0.002, standardise=True)
    print("shifted by 5 m: joint", sat["joint"], "floor", sat["floor"])
    assert abs(sat["joint"] - sat["floor"]) <= 1e-6
    far = solver.posterior_mmd(shifted, first, estimator="MMDb")
    pose0 = next(v for v in order if v.name == "X0")
    print("shifted by 5 m at the default bandwidth:", far["joint"], {v.name: a for v, a in far["marginal"].items()})
    assert far["marginal"][pose0] > 1.0 and far["joint"] > far["floor"]

    # the device draw scored where it lies == the same points handed over (also as a block of two variables, all columns)
    torch.manual_seed(17)
    lying = solver.posterior_mmd(second, n=300, blocks=[(order[0], order[-1])], columns="all", estimator="MMDb")
    torch.manual_seed(17)
    drawn = solver.posterior_collect(solver.posterior_launch(300))
    given = solver.posterior_mmd(second, drawn, blocks=[(order[0], order[-1])], columns="all", estimator="MMDb")
    assert lying["n"] == 300 and lying["m"] == n and len(lying["blocks"]) == 1
    assert lying["joint"] == given["joint"] and lying["marginal"] == given["marginal"] and lying["blocks"] == given["blocks"]
    assert lying["marginal_mean"] == np.mean([lying["marginal"][v] for v in order])

    # one variable's marginal is mmd_blocks on that variable's columns
    for v in order:
        want = ST.mmd_blocks(first[v], second[v], [[0, 1]], estimator="mmd", device=DEV)[0]
        got = own["marginal"][v]
        assert (np.isnan(want) and np.isnan(got)) or got == want, (v, got, want)
    pose = next(v for v in order if v.dim == 3)
    allc = solver.posterior_mmd(second, first, variables=[pose], columns="all", estimator="MMDb", joint=False)
    want = ST.mmd_blocks(first[pose], second[pose], [[0, 1, 2]], circular=[False, False, True], device=DEV)[0]
    assert allc["joint"] is None and allc["marginal"][pose] == want
