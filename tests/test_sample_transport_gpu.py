"""The sliced Wasserstein distance on the GPU (nfisam_sample_sliced_transport through nfisam_hip.sliced_transport,
utils.Statistics.sliced_wasserstein and NFiSAM.posterior_transport).

The oracle is the float64 numpy evaluation of tests/test_sample_transport_cpu.py at the same float32 points, directions and
scales (`oracle_slices`: keys summed in ascending entry order, `np.sort`, the pieces between neighbouring cuts of the two
quantile functions).  Tolerance per slice, derived there (`tolerance`), not measured:
    |dev - ref| <= 4 [ 2 p (d + 1) eps A1 ref^((p - 1) / p) + (m + n) eps ref ],   eps = 2^-52,
A1 the largest sum_e |dir scale f(x)| over the points (the oracle computes it).  The largest observed ratio to that bound is
printed per test; an MI355X's are in profiles/sample_transport.json (`tolerance_ratio`; written by running this file as a
script, see `write_profile`) and quoted in DESIGN.md 3.3q."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_transport_cpu import COLS, arrays, directions, fixture, oracle_keys, oracle_slices, table, tolerance
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 3), (64, 64), (65, 64), (130, 200), (257, 255)]
RATIOS = {}


def _ratio(dev, ref, tol):
    """max |dev - ref| / tol; where the bound is 0 (ref = 0 exactly) the device value must be 0 too."""
    dev, ref, tol = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (dev, ref, tol))
    err = np.abs(dev - ref)
    assert np.all(np.isfinite(dev)), dev
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))))


def _record(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("largest |dev - ref| / bound, %s: %.3g" % (name, ratio))


def _split(out, blocks):
    out = out.cpu().numpy() if torch.is_tensor(out) else out
    return [out[int(b["out_off"]):int(b["out_off"]) + int(b["n_dirs"])] for b in blocks]


def _run(x, y, tab, p, dirs=None):
    blocks, xcols, ycols, flat, kind, scale = arrays(tab, dirs)
    return _split(nh.sliced_transport(x, y, blocks, xcols, ycols, flat, p, kind, scale, device=DEV), blocks)


def _oracle_ratio(x, y, tab, p, got, dirs=None):
    dirs = directions(tab) if dirs is None else dirs
    worst = 0.0
    for b, D, g in zip(tab, dirs, got):
        ref, a1 = oracle_slices(x, y, b[0], b[1], D, p, b[4], b[3])
        worst = max(worst, _ratio(g, ref, tolerance(ref, p, len(b[0]), a1, x.shape[0], y.shape[0])))
    return worst


# ---- against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("m,n", SHAPES)
def test_slices_follow_the_oracle(m, n, p):
    """All ten blocks of the table (d in {1, 2, 7, 17, 40}, 1 / 5 / 64 directions, a scale, xcols != ycols, headings either
    side of the seam, tied rows) in one launch, at every shape where the kernel takes another path: one point, pad == size,
    pads 128 / 64, gcd 10, coprime sizes with pads 512 / 256 across the 256-thread stride."""
    x, y = fixture(m, n)
    tab = table()
    got = _run(x, y, tab, p)
    ratio = _oracle_ratio(x, y, tab, p, got)
    _record("oracle_m%d_n%d_p%d" % (m, n, p), ratio)
    assert ratio <= 1.0


def test_the_lds_cap():
    """m = n = 8192: 128 KiB of keys, the one launch above 48 KiB and the reason the entry sets the dynamic-LDS attribute."""
    x, y = fixture(nh.TRANSPORT_MAX_N, nh.TRANSPORT_MAX_N, seed=35)
    tab = [([1, 2], [1, 2], 2, None, None)]
    for p in (1, 2):
        got = _run(x, y, tab, p)
        ratio = _oracle_ratio(x, y, tab, p, got)
        _record("lds_cap_p%d" % p, ratio)
        assert ratio <= 1.0


def test_statistics_front_and_the_axes():
    """`sliced_wasserstein` with circular columns, a scale and axes: its slices are the oracle's at `transport_directions`,
    the axis values are the exact 1-D distances of the entries, and the column-major form gives the same bits."""
    x, y = fixture(130, 200)
    circ = np.zeros(COLS, dtype=bool)
    circ[40:42] = True
    scale = np.ones(COLS)
    scale[3] = 0.5
    blocks = [[0], [3, 4, 40], ([9, 10], [10, 9]), [41]]
    for p in (1, 2):
        res = ST.sliced_wasserstein(x, y, blocks, p=p, directions=5, seed=3, scale=scale, circular=circ, axes=True, device=DEV)
        tab = [([0], [0], 1, None, None), ([3, 4, 40, 40], [3, 4, 40, 40], 5, [0.5, 1.0, 1.0, 1.0], [0, 0, 1, 2]),
               ([9, 10], [10, 9], 5, None, None), ([41, 41], [41, 41], 5, None, [1, 2])]
        worst = _oracle_ratio(x, y, tab, p, res["slices"], [ST.transport_directions(len(b[0]), 5, 3) for b in tab])
        for b, ax, s in zip(tab, res["axis"], res["slices"]):
            assert len(ax) == len(b[0]) and len(s) == (1 if len(b[0]) == 1 else 5)
            for e in range(len(b[0])):
                sc = None if b[3] is None else [b[3][e]]
                ref, a1 = oracle_slices(x, y, [b[0][e]], [b[1][e]], np.ones((1, 1)), p, None if b[4] is None else [b[4][e]], sc)
                worst = max(worst, _ratio(ax[e] ** p, ref, tolerance(ref, p, 1, a1, 130, 200)))
        _record("front_p%d" % p, worst)
        assert worst <= 1.0
        assert res["distance"][0] == res["max_sliced"][0]             # a one-entry block: one direction, its own axis
        assert abs(res["axis"][0][0] - res["distance"][0]) <= 4 * 2.0 ** -52 * res["distance"][0]
        for b in range(4):
            assert (res["distance"][b], res["max_sliced"][b]) == ST.wasserstein_from_slices(res["slices"][b], p)
        Xt, Yt = nh._columns(x, DEV), nh._columns(y, DEV)
        again = ST.sliced_wasserstein_t(Xt, Yt, blocks, p=p, directions=5, seed=3, scale=scale, circular=circ, axes=True)
        assert all(np.array_equal(a, b) for a, b in zip(res["slices"], again["slices"]))
        assert all(np.array_equal(a, b) for a, b in zip(res["axis"], again["axis"]))


# ---- exact identities -----------------------------------------------------------------------------------------------------------
def _same_columns(tab):
    return [b for b in tab if b[0] == b[1]]


@pytest.mark.parametrize("p", [1, 2])
def test_a_permuted_and_a_repeated_set_are_at_distance_exactly_zero(p):
    x, _ = fixture(130, 200)
    tab = _same_columns(table())
    perm = np.random.RandomState(5).permutation(130)
    twice = np.concatenate([x, x])[np.random.RandomState(6).permutation(260)]
    for a, y in ((x, x[perm]), (x, twice), (twice, x), (x[:65], x[:65].repeat(3, axis=0))):
        for b, s in zip(tab, _run(a, y, tab, p)):
            assert np.all(s == 0.0) and not np.any(np.signbit(s)), (b, s)


@pytest.mark.parametrize("p", [1, 2])
def test_an_exact_shift_moves_every_slice_by_its_projection(p):
    """X on a grid of eighths near 100, Y = X + 1/2 (exact in float32), m = n: every key moves by c * sum(theta), the order
    statistics pair up, so the slice is |c sum_e theta_e scale_e|^p."""
    rng = np.random.RandomState(8)
    x = (100.0 + rng.randint(-40, 40, size=(96, COLS)) / 8.0).astype(np.float32)
    y = (x.astype(np.float64) + 0.5).astype(np.float32)
    assert np.array_equal(y.astype(np.float64) - x.astype(np.float64), np.full(x.shape, 0.5))
    tab = [b for b in _same_columns(table()) if b[4] is None]
    dirs = directions(tab)
    worst = 0.0
    for b, D, s in zip(tab, dirs, _run(x, y, tab, p, dirs)):
        sc = np.ones(len(b[0])) if b[3] is None else np.asarray(b[3])
        ref = np.abs(0.5 * (D * sc[None, :]).sum(1)) ** p
        a1 = max(oracle_keys(x, b[0], D, None, b[3])[1], oracle_keys(y, b[1], D, None, b[3])[1])
        worst = max(worst, _ratio(s, ref, tolerance(ref, p, len(b[0]), a1, 96, 96)))
    _record("shift_p%d" % p, worst)
    assert worst <= 1.0


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_twice_alone_reversed_and_per_direction():
    x, y = fixture(130, 200)
    tab = table()
    dirs = directions(tab)
    for p in (1, 2):
        full = _run(x, y, tab, p, dirs)
        assert all(np.array_equal(a, b) for a, b in zip(full, _run(x, y, tab, p, dirs)))                  # a second call
        for k, b in enumerate(tab):                                                                      # each block alone
            assert np.array_equal(_run(x, y, [b], p, [dirs[k]])[0], full[k]), k
        rev = _run(x, y, tab[::-1], p, dirs[::-1])[::-1]                                                 # the table reversed
        assert all(np.array_equal(a, b) for a, b in zip(full, rev))
        twice = _run(x, y, [tab[2], tab[4], tab[2]], p, [dirs[2], dirs[4], dirs[2]])                     # a block repeated
        assert np.array_equal(twice[0], full[2]) and np.array_equal(twice[2], full[2]) and np.array_equal(twice[1], full[4])
        for k, j in ((2, 37), (4, 63), (4, 0), (7, 11)):                                                 # one direction alone
            one = (tab[k][0], tab[k][1], 1, tab[k][3], tab[k][4])
            assert _run(x, y, [one], p, [dirs[k][j:j + 1]])[0][0] == full[k][j], (k, j)


# ---- the C entry given a bad device table -----------------------------------------------------------------------------------------
def test_a_bad_device_table_yields_nan_in_its_own_slices_only():
    """The binding refuses these tables; the C entry cannot (it does not read device arrays on the host): a block whose
    entries leave the lists, one that names a row outside its matrix (either matrix, either side of the range) and one with
    kind 3 give NaN in exactly their slices, and the good blocks between them the bits of a good run."""
    x, y = fixture(130, 200)
    good = [([1, 2], [1, 2], 5, None, None), (list(range(3, 10)), list(range(3, 10)), 64, None, None),
            ([3, 4, 40, 40], [3, 4, 40, 40], 5, None, [0, 0, 1, 2])]
    gdirs = directions(good)
    want = _run(x, y, good, 2, gdirs)
    # good0 | entries leave | good1 | xcols row == x_rows | ycols row == -1 | kind 3 | good2
    tab = [good[0], ([0, 1], [0, 1], 5, None, None), good[1], ([2, COLS, 4], [2, 3, 4], 5, None, None),
           ([2, 3, 4], [2, -1, 4], 5, None, None), ([5, 6], [5, 6], 5, None, [0, 3]), good[2]]
    dirs = [gdirs[0], ST.transport_directions(2, 5, 0), gdirs[1], ST.transport_directions(3, 5, 0), ST.transport_directions(3, 5, 0),
            ST.transport_directions(2, 5, 0), gdirs[2]]
    blocks, xcols, ycols, flat, kind, _ = arrays(tab, dirs)
    ne = int(xcols.size)
    blocks["col_off"][1], blocks["d"][1] = ne - 1, 2                               # one entry past the end of the lists
    n_out = int(blocks["n_dirs"].sum())
    Xt, Yt = nh._columns(x, DEV), nh._columns(y, DEV)
    dev = nh._upload_named(DEV, blocks=nh._table_bytes(blocks), xcols=xcols, ycols=ycols, kind=kind, dirs=flat)
    out = torch.full((n_out,), 7.0, dtype=torch.float64, device=DEV)
    rc = nh.lib().nfisam_sample_sliced_transport(nh._ptr(Xt), COLS, 130, nh._ptr(Yt), COLS, 200, blocks.ctypes.data_as(C.c_void_p),
                                                 nh._ptr(dev["blocks"]), len(tab), nh._ptr(dev["xcols"]), nh._ptr(dev["ycols"]),
                                                 nh._ptr(dev["kind"]), None, ne, nh._ptr(dev["dirs"]), int(flat.size), 2,
                                                 nh._ptr(out), n_out, nh._stream())
    assert rc == nh.OK
    got = _split(out, blocks)
    for k in (1, 3, 4, 5):
        assert np.all(np.isnan(got[k])), (k, got[k])
    for k, w in zip((0, 2, 6), want):
        assert np.array_equal(got[k], w), k


# ---- the solver -------------------------------------------------------------------------------------------------------------------
def _block_oracle(own, ref, blk, p, directions_count=64, seed=0):
    """-> (mean of the oracle's slices, mean of their tolerances) of the xy block `blk` (a tuple of variables)."""
    X = np.concatenate([np.asarray(own[v])[:, :2] for v in blk], axis=1)
    Y = np.concatenate([np.asarray(ref[v])[:, :2] for v in blk], axis=1)
    d = X.shape[1]
    D = ST.transport_directions(d, directions_count, seed)
    s, a1 = oracle_slices(X, Y, list(range(d)), list(range(d)), D, p)
    return s, tolerance(s, p, d, a1, X.shape[0], Y.shape[0])


def test_posterior_transport_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem, then a stored draw against (a) itself: every number exactly 0; (b) itself with
    one landmark moved by (0.5, 0): that landmark's marginal, its first axis and every block that holds it follow the oracle,
    every other marginal is exactly 0; and a draw made by the call: finite values under the right keys."""
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
    n = len(first[order[0]])
    lm = next(v for v in order if v.dim == 2)
    pose = next(v for v in order if v.dim == 3)

    def no_draw(*a, **k):
        raise AssertionError("drawn although samples were given")
    solver.posterior_launch = no_draw                                 # (on the instance: deleted again below)
    for p in (1, 2):
        same = solver.posterior_transport(first, first, p=p, blocks=[(pose, lm)])
        assert same["joint"] == 0.0 and same["marginal_mean"] == 0.0 and same["marginal_max"] == 0.0 and same["blocks"] == [0.0]
        assert set(same["marginal"]) == set(order) and all(a == 0.0 for a in same["marginal"].values())
        assert set(same["max_sliced"]) == set(order) | {"joint"} and all(a == 0.0 for a in same["max_sliced"].values())
        assert all(np.all(a == 0.0) and len(a) == 2 for a in same["axes"].values())
        assert (same["m"], same["n"], same["p"], same["directions"]) == (n, n, p, 64)

        moved = dict(first)
        moved[lm] = first[lm] + np.array([0.5, 0.0])
        res = solver.posterior_transport(moved, first, p=p, blocks=[(pose, lm), (pose,)])
        worst = 0.0
        for got, blk in ((res["marginal"][lm], (lm,)), (res["joint"], tuple(order)), (res["blocks"][0], (pose, lm))):
            s, tol = _block_oracle(first, moved, blk, p)
            worst = max(worst, _ratio(got ** p, s.mean(), tol.mean() + 4 * 2.0 ** -52 * s.mean()))
            assert 0.0 < got <= 0.5 * (1 + 1e-4)                                     # a slice moves by |0.5 theta_x| <= 0.5
        s, tol = _block_oracle(first, moved, (lm,), p)
        worst = max(worst, _ratio(res["max_sliced"][lm] ** p, s.max(), tol.max()))
        X = np.asarray(first[lm])[:, :1]
        ref, a1 = oracle_slices(X, np.asarray(moved[lm])[:, :1], [0], [0], np.ones((1, 1)), p)
        worst = max(worst, _ratio(res["axes"][lm][0] ** p, ref, tolerance(ref, p, 1, a1, n, n)))
        _record("solver_p%d" % p, worst)
        assert worst <= 1.0
        assert abs(res["axes"][lm][0] - 0.5) <= 1e-4 and res["axes"][lm][1] == 0.0   # (0.5 up to the float32 rounding of the sum)
        assert all(res["marginal"][v] == 0.0 and np.all(res["axes"][v] == 0.0) for v in order if v is not lm)
        assert res["blocks"][1] == 0.0 and res["marginal_max"] == res["marginal"][lm]
        assert res["marginal_mean"] == np.mean([res["marginal"][v] for v in order])
    allc = solver.posterior_transport(first, first, variables=[pose], columns="all", joint=False, axes=False)
    assert allc["joint"] is None and allc["axes"] is None and allc["marginal"] == {pose: 0.0} and set(allc["max_sliced"]) == {pose}
    del solver.posterior_launch

    torch.manual_seed(17)
    drawn = solver.posterior_transport(first, n=300, columns="all")
    assert (drawn["m"], drawn["n"], drawn["p"], drawn["directions"]) == (n, 300, 2, 64) and drawn["blocks"] == []
    assert set(drawn["marginal"]) == set(order) and set(drawn["axes"]) == set(order)
    assert all(len(drawn["axes"][v]) == (4 if v.dim == 3 else 2) for v in order)
    vals = [drawn["joint"], drawn["marginal_mean"], drawn["marginal_max"]] + list(drawn["marginal"].values()) + \
        list(drawn["max_sliced"].values()) + [float(a) for v in order for a in drawn["axes"][v]]
    assert all(np.isfinite(a) and a >= 0.0 for a in vals), vals
    assert all(drawn["marginal"][v] <= drawn["max_sliced"][v] for v in order)
    default = solver.posterior_transport(first)
    assert default["n"] == n and np.isfinite(default["joint"])


def write_profile(path):
    """The largest observed ratio to the bound per test -> `tolerance_ratio` of the JSON at `path` (other keys are kept).
    From the repository root, on an MI355X:
        PYTHONPATH=nf-isam_amd:.:tests python tests/test_sample_transport_gpu.py profiles/sample_transport.json"""
    import tempfile
    from pathlib import Path
    for m, n in SHAPES:
        for p in (1, 2):
            test_slices_follow_the_oracle(m, n, p)
    test_the_lds_cap()
    test_statistics_front_and_the_axes()
    for p in (1, 2):
        test_an_exact_shift_moves_every_slice_by_its_projection(p)
    with tempfile.TemporaryDirectory() as tmp:
        test_posterior_transport_on_the_small_range_problem(Path(tmp))
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["tolerance_ratio"] = dict(device=torch.cuda.get_device_name(0), bound="4 [2 p (d + 1) eps A1 ref^((p-1)/p) + (m + n) eps ref]",
                                  largest=max(RATIOS.values()), per_test={k: RATIOS[k] for k in sorted(RATIOS)})
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("largest ratio %.3g -> %s" % (max(RATIOS.values()), path))


if __name__ == "__main__":
    write_profile(sys.argv[1])
