"""The sample summaries on the device against the float64 oracle of tests/test_sample_summary_cpu.py (every sum by math.fsum:
the oracle's own summation error is one rounding, so each comparison bounds the device alone).

Bounds (u = 2^-53, ulp = 2^-52, n points, s_e = max_i |r_e,i| from the oracle); none of them is fitted to an output:
  Euclidean mean  |d| <= 4 n u max|x|.  The device forms x_0 + sum w (x - x_0) / W.  Its sums are 256 strided partial sums, a
                  6-level tree and 3 more additions: at most min(n - 1, ceil(n / 256) + 9) additions deep, one product
                  rounding per term, |x - x_0| <= 2 max|x|; with the rounding of W (same depth), of the division and of the
                  final addition that is at most (2 (depth + 2) + 3) u max|x|, which is below 4 n u max|x| for every n >= 2
                  used here (n = 2: 7 u against 8 u); at n = 1 the sum is exactly 0 and the mean exactly x_0.
  resultant       |d| <= 4 n u + 8 u   (cos and sin good to about 2 ulp, the sum bound as above on terms <= 1).
  circular mean   |d| <= (4 n u + 8 u) / R + 4 u pi wherever the oracle's R >= 0.1 (asserted for the concentrated heading);
                  a heading without direction need only be finite and meet the resultant bound.
  covariance      |d| <= 1e-11 s_e s_f + 1e-300  (accumulation <= 8 n u = 2.7e-13 at n = 300; a circular column's mean shift
                  adds at most dmean * s).  For the directionless heading dmean <= (4 n u + 8 u) / R, which stays below 1e-11
                  while R >= 0.02: asserted on the oracle for every n used.  The constant column: exactly 0.
  quantiles       where p (n - 1) is an integer: the sorted key, bit for bit; elsewhere |d| <= 6 ulp(max(|a|, |b|)) of the two
                  neighbouring keys (max(|a|, |b|, pi) for a heading: the centre is added back) + 4 ulp(max(h, 1)) |b - a|.
                  The second term corrects the derivation the first came from ("two float64 lerps of exact keys"): the
                  position h is not exact on either side.  The device rounds h = p (n - 1) once (<= u h); np.quantile forms
                  the same number as (n p + (1 - p)) - 1, three roundings (<= u n p + u (n p + 1) + u); the two positions
                  differ by up to 3 u (h + 4/3) <= 4 ulp(max(h, 1)), and the interpolation carries that into the value
                  times the gap |b - a|.  Seen at n = 256, p = 0.95 on the column of half-integer ties: h = 242.24999999999997
                  here, 242.25 in numpy, the values 5.8e-15 apart across a gap of 0.5 -- against 2.7e-15 for the first term
                  alone.  Where the gap is small against the keys, as for continuous data, the term vanishes.

Largest measured excess over a bound on MI355X: none for the moments -- the largest error / bound over all cases was 0.0050
(Euclidean mean), 0.0077 (resultant), 0.014 (circular mean), 2.0e-5 (covariance).  The interpolated quantiles exceeded the
first term of their bound once, by 2.2 x (the case above, 5.8e-15 against 2.7e-15); with the corrected derivation the largest
error / bound is 0.17 (profiles/r11_sample_summary.json, `largest_deviation`)."""
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_summary_cpu import fixture_case, oracle_moments, oracle_quantiles, wrap_pi
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
ROWS, COLS = 300, 40
U = 2.0 ** -53
HEADING, UNIFORM, CONSTANT, TIES, FAR = 6, 7, 8, 9, 2          # columns of _data()
NS = [1, 2, 63, 64, 65, 255, 256, 257, 300]
PROBS = [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0]


def _data():
    rng = np.random.RandomState(20241018)
    x = np.empty((ROWS, COLS))
    offsets, spreads = [0.0, 3.0, 100.0], [1.5, 0.01]
    for c in range(COLS):
        x[:, c] = rng.standard_normal(ROWS) * spreads[(c // 3) % 2] + offsets[c % 3]
    # column 2 (FAR) is offset 100 with spread 1.5 so far: make it the one a one-pass variance would fail
    x[:, FAR] = rng.standard_normal(ROWS) * 0.01 + 100.0
    x[:, HEADING] = wrap_pi(rng.standard_normal(ROWS) * 0.2 + 3.0)          # mass on both sides of +-pi
    x[:, UNIFORM] = rng.uniform(-np.pi, np.pi, ROWS)
    x[:, CONSTANT] = 7.25
    x[:, TIES] = np.round(rng.standard_normal(ROWS) * 1.5 * 2.0) / 2.0      # many equal values
    return x.astype(np.float32)


def _weights():
    w = np.random.RandomState(7).uniform(size=ROWS)
    w[5::10] = 0.0                                                           # a tenth exactly zero (never the first two)
    return w


def _table():
    """[(columns, circular flags)]"""
    t = [[0], [1, FAR], [0, 1, HEADING], [9, 10, 11, 12, 13], [0, 1, HEADING, 3, 4, UNIFORM], list(range(10, 26)), [FAR, FAR],
         [39, 5, 17, CONSTANT], [FAR, CONSTANT], [CONSTANT], [UNIFORM], [HEADING], [TIES, 30, 31]]
    return [(cols, [c in (HEADING, UNIFORM) for c in cols]) for cols in t]


def _arrays(table):
    blocks = nh.pack_moment_blocks([len(c) for c, _ in table])
    cols = np.concatenate([np.asarray(c) for c, _ in table]).astype(np.int32)
    circ = np.concatenate([np.asarray(f) for _, f in table]).astype(np.uint8)
    return blocks, cols, circ


def _run(x, table, weights=None):
    blocks, cols, circ = _arrays(table)
    mean, res, cov = nh.sample_moments(x, blocks, cols, circular=circ, weights=weights, device=DEV)
    return blocks, mean.cpu().numpy(), res.cpu().numpy(), cov.cpu().numpy()


_worst = {}


def _note(kind, err, bound):
    ratio = float(np.max(np.asarray(err) / np.asarray(bound))) if np.size(err) else 0.0
    _worst[kind] = max(_worst.get(kind, 0.0), ratio)
    return ratio


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", NS)
def test_moments_match_the_float64_oracle(n, weighted):
    x = _data()[:n]
    w = _weights()[:n] if weighted else None
    table = _table()
    blocks, mean, res, cov = _run(x, table, w)
    x64 = x.astype(np.float64)
    for (cols, flags), row in zip(table, blocks):
        o, d, c = int(row["col_off"]), int(row["d"]), int(row["cov_off"])
        m_o, r_o, cov_o, s = oracle_moments(x, cols, flags, w)
        got_m, got_r, got_c = mean[o:o + d], res[o:o + d], cov[c:c + d * d].reshape(d, d)
        for e, (col, circ) in enumerate(zip(cols, flags)):
            if circ:
                rb = 4 * n * U + 8 * U
                print("n", n, "col", col, "resultant", got_r[e], r_o[e], "ratio", _note("resultant", abs(got_r[e] - r_o[e]), rb))
                assert abs(got_r[e] - r_o[e]) <= rb, (n, col, got_r[e], r_o[e])
                if col == HEADING:
                    assert r_o[e] >= 0.1
                if col == UNIFORM and n >= 2:
                    assert r_o[e] >= 0.02                      # (what the covariance bound's derivation needs: see above)
                assert np.isfinite(got_m[e]) and -np.pi <= got_m[e] < np.pi
                if r_o[e] >= 0.1:
                    mb = rb / r_o[e] + 4 * U * np.pi
                    print("n", n, "col", col, "circular mean", got_m[e], m_o[e], "ratio", _note("circular_mean", abs(got_m[e] - m_o[e]), mb))
                    assert abs(got_m[e] - m_o[e]) <= mb, (n, col, got_m[e], m_o[e])
            else:
                mb = 4 * n * U * np.abs(x64[:, col]).max()
                print("n", n, "col", col, "mean", got_m[e], m_o[e], "ratio", _note("mean", abs(got_m[e] - m_o[e]), mb))
                assert abs(got_m[e] - m_o[e]) <= mb, (n, col, got_m[e], m_o[e])
                assert np.isnan(got_r[e])
                if col == CONSTANT:
                    assert got_m[e] == 7.25 and got_c[e, e] == 0.0 and np.all(got_c[e, :] == 0.0)
        cb = 1e-11 * np.outer(s, s) + 1e-300
        print("n", n, "block", cols, "cov ratio", _note("cov", np.abs(got_c - cov_o), cb))
        assert np.all(np.abs(got_c - cov_o) <= cb), (n, cols, got_c, cov_o)
        assert np.array_equal(got_c, got_c.T)
    print("largest error / bound so far:", json.dumps(_worst))


def test_the_far_narrow_column_is_what_a_one_pass_variance_fails():
    """Offset 100, spread 0.01: sum x^2 / n - mean^2 in float64 loses what the two-pass device value keeps."""
    x = _data()
    _, _, _, cov = _run(x, [([FAR], [False])])
    _, _, cov_o, s = oracle_moments(x, [FAR])
    x64 = x[:, FAR].astype(np.float64)
    one_pass = (x64 * x64).sum() / ROWS - (x64.sum() / ROWS) ** 2
    bound = 1e-11 * s[0] * s[0]
    print("device", cov[0], "oracle", cov_o[0, 0], "one pass", one_pass, "bound", bound)
    assert abs(cov[0] - cov_o[0, 0]) <= bound < abs(one_pass - cov_o[0, 0])


def test_second_call_single_blocks_reversed_table_and_shared_columns_give_the_same_bits():
    x, w = _data(), _weights()
    table = _table()
    for weights in (None, w):
        blocks, mean, res, cov = _run(x, table, weights)
        again = _run(x, table, weights)
        assert np.array_equal(mean, again[1]) and np.array_equal(res, again[2], equal_nan=True) and np.array_equal(cov, again[3])
        rb, rmean, rres, rcov = _run(x, table[::-1], weights)
        k = len(table)
        for i, ((cols, flags), row) in enumerate(zip(table, blocks)):
            o, d, c = int(row["col_off"]), int(row["d"]), int(row["cov_off"])
            _, m1, r1, c1 = _run(x, [(cols, flags)], weights)
            ro, rc = int(rb[k - 1 - i]["col_off"]), int(rb[k - 1 - i]["cov_off"])
            for m2, r2, c2 in ((m1, r1, c1), (rmean[ro:ro + d], rres[ro:ro + d], rcov[rc:rc + d * d])):
                assert np.array_equal(mean[o:o + d], m2) and np.array_equal(res[o:o + d], r2, equal_nan=True)
                assert np.array_equal(cov[c:c + d * d], c2), (i, cols)
        # a column has the same mean bits in every block that holds it, a pair of columns the same covariance bits
        _, cols_flat, _ = _arrays(table)
        for col in (0, 1, FAR, HEADING, CONSTANT, UNIFORM):
            assert len(set(mean[cols_flat == col].tolist())) == 1, col
        pose, two = blocks[2], blocks[4]                       # [0, 1, HEADING] and [0, 1, HEADING, 3, 4, UNIFORM]
        a = cov[int(pose["cov_off"]):int(pose["cov_off"]) + 9].reshape(3, 3)
        b = cov[int(two["cov_off"]):int(two["cov_off"]) + 36].reshape(6, 6)
        assert np.array_equal(a, b[:3, :3])
        rep = cov[int(blocks[6]["cov_off"]):int(blocks[6]["cov_off"]) + 4]               # [FAR, FAR]: one value four times
        assert len(set(rep.tolist())) == 1
    ones = _run(x, table, np.ones(ROWS))                                          # NULL weights are all ones
    none = _run(x, table, None)
    assert np.array_equal(ones[1], none[1]) and np.array_equal(ones[3], none[3])


def _quantile_columns():
    return [0, FAR, HEADING, UNIFORM, CONSTANT, TIES, 5, 39], [False, False, True, True, False, False, False, False]


@pytest.mark.parametrize("n", NS + [127, 128, 129])
def test_quantiles_match_numpy_on_the_sorted_keys(n):
    x = _data()[:n]
    cols, flags = _quantile_columns()
    center = np.array([oracle_moments(x, [c], [f])[0][0] if f else 0.0 for c, f in zip(cols, flags)])
    got = nh.sample_quantiles(x, cols, PROBS, circular=np.asarray(flags, dtype=np.uint8), center=center, device=DEV).cpu().numpy()
    again = nh.sample_quantiles(x, cols, PROBS, circular=np.asarray(flags, dtype=np.uint8), center=center, device=DEV).cpu().numpy()
    assert got.shape == (len(cols), len(PROBS)) and np.array_equal(got, again)
    for e, (col, circ) in enumerate(zip(cols, flags)):
        want, s = oracle_quantiles(x, col, PROBS, circ, center[e])
        if circ:
            assert np.all(np.abs(np.abs(s) - np.pi) > 1e-6)                       # no key near the cut
        for q, p in enumerate(PROBS):
            h = p * (n - 1)
            lo, hi = int(np.floor(h)), int(np.ceil(h))
            if lo == h:
                exact = s[lo] + center[e] if circ else s[lo]
                assert got[e, q] == exact, (n, col, p, got[e, q], exact)
            else:
                scale = max(abs(s[lo]), abs(s[hi]), np.pi if circ else 0.0)
                bound = 6 * np.spacing(scale) + 4 * np.spacing(max(h, 1.0)) * abs(s[hi] - s[lo])
                ratio = _note("quantile", abs(got[e, q] - want[q]), bound) if bound > 0 else 0.0
                print("n", n, "col", col, "p", p, got[e, q], want[q], "ratio", ratio)
                assert abs(got[e, q] - want[q]) <= bound, (n, col, p, got[e, q], want[q])
        assert np.all(np.diff(got[e]) >= 0)                                       # a heading's are unwrapped: still ordered
        if col in (CONSTANT,):
            assert np.all(got[e] == 7.25)
    one = nh.sample_quantiles(x, [cols[2]], PROBS, circular=[1], center=center[2:3], device=DEV).cpu().numpy()
    assert np.array_equal(one[0], got[2])                                         # alone == in the table
    print("largest error / bound so far:", json.dumps(_worst))


def test_a_bad_block_given_to_the_c_entry_yields_nan_and_leaves_the_others_alone():
    """`checked=True` skips the binding's table check: the C entry sees a row past x_rows, a negative row and a block that
    runs past n_entries.  The reads stay in bounds by construction (row 0 stands in, the block is not walked)."""
    x = _data()
    table = _table()[:6]
    blocks, cols, circ = _arrays(table)
    Xt = torch.from_numpy(x.T.copy()).to(DEV)
    good = [t.cpu().numpy() for t in nh.sample_moments_t(Xt, blocks, cols, circ)]

    def block_cov(cov, b):
        return cov[int(blocks[b]["cov_off"]):int(blocks[b]["cov_off"]) + int(blocks[b]["d"]) ** 2]

    for bad_row in (COLS, -1):
        bad = cols.copy()
        bad[2] = bad_row                                       # entry 2 = the second column of block 1 (entries 1..2)
        mean, res, cov = (t.cpu().numpy() for t in nh.sample_moments_t(Xt, blocks, bad, circ, checked=True))
        keep = np.arange(cols.size) != 2
        assert np.isnan(mean[2]) and np.isnan(res[2])
        assert np.array_equal(mean[keep], good[0][keep]) and np.array_equal(res[keep], good[1][keep], equal_nan=True)
        assert np.all(np.isnan(block_cov(cov, 1)))
        for b in (0, 2, 3, 4, 5):
            assert np.array_equal(block_cov(cov, b), block_cov(good[2], b)), b
        q = nh.sample_quantiles_t(Xt, bad[:4], PROBS, checked=True).cpu().numpy()
        qg = nh.sample_quantiles_t(Xt, cols[:4], PROBS).cpu().numpy()
        assert np.all(np.isnan(q[2])) and np.array_equal(q[[0, 1, 3]], qg[[0, 1, 3]])
    past = blocks.copy()
    past["col_off"][5] = int(cols.size) - 15                   # d = 16: runs one entry past the list
    mean, res, cov = (t.cpu().numpy() for t in nh.sample_moments_t(Xt, past, cols, circ, checked=True))
    assert np.all(np.isnan(block_cov(cov, 5))) and np.array_equal(mean, good[0])
    for b in range(5):
        assert np.array_equal(block_cov(cov, b), block_cov(good[2], b)), b
    with pytest.raises(ValueError):                                               # the binding's own check refuses them
        nh.sample_moments_t(Xt, past, cols, circ)
    with pytest.raises(ValueError):
        nh.sample_moments_t(Xt, blocks, bad, circ)
    with pytest.raises(ValueError):
        nh.sample_quantiles_t(Xt, bad[:4], PROBS)


def test_quantiles_at_the_cap():
    """n = 16384 takes 128 KiB of LDS (raised above the default limit); one more point is refused before any launch."""
    rng = np.random.RandomState(11)
    x = rng.standard_normal((nh.QUANTILE_MAX_N, 2)).astype(np.float32)
    got = nh.sample_quantiles(x, [0, 1], [0.0, 0.5, 1.0], device=DEV).cpu().numpy()
    for c in range(2):
        s = np.sort(x[:, c].astype(np.float64))
        assert got[c, 0] == s[0] and got[c, 2] == s[-1]
        assert abs(got[c, 1] - np.quantile(s, 0.5)) <= 6 * np.spacing(max(abs(s[8191]), abs(s[8192])))
    with pytest.raises(ValueError, match="16384"):
        nh.sample_quantiles(np.zeros((nh.QUANTILE_MAX_N + 1, 1), dtype=np.float32), [0], [0.5], device=DEV)


# ---- pinned to the reference --------------------------------------------------------------------------------------------------
def test_sample_mean_equals_the_reference_values():
    """tests/golden/sample_summary.npz: the reference's own `sample_mean` (np.mean and scipy's circmean, whose pairwise sums
    err too: twice the bounds above)."""
    fx = np.load(os.path.join(GOLDEN, "sample_summary.npz"))
    for k in range(int(fx["n_cases"])):
        variables, x, means, var2mean, _ = fixture_case(fx, k)
        got, got_map = ST.sample_mean(torch.from_numpy(x).to(DEV), variables)
        n = x.shape[0]
        flags = [bool(c) for v in variables for c in v.circular_dim_list]
        assert got.shape == means.shape and list(got_map) == variables
        for c, circ in enumerate(flags):
            if circ:
                R = oracle_moments(x, [c], [True])[1][0]
                assert R >= 0.1
                bound = 2 * ((4 * n * U + 8 * U) / R + 4 * U * np.pi)
            else:
                bound = 2 * 4 * n * U * np.abs(x[:, c].astype(np.float64)).max()
            print(k, c, circ, got[c], means[c], abs(got[c] - means[c]), bound)
            assert abs(got[c] - means[c]) <= bound, (k, c, got[c], means[c])
        at = 0
        for v in variables:
            assert np.array_equal(got_map[v], got[at:at + v.dim])
            at += v.dim


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def test_posterior_summary_on_the_small_range_problem(tmp_path):
    """Two updates of the small range problem (the fixture and seeds of the MMD solver test).  The importance-weighted
    summary is compared with the same call given exp(log w - max) from `posterior_diagnostics` at 1e-12 relative to the scale
    of the summed terms (max|x| of the column for a mean, s_e s_f for a covariance -- the scales of the bounds above): the two
    weight vectors differ by the last bits of two exp implementations, a mean near zero has no scale of its own."""
    from scipy.stats import circmean
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
    n = 300

    # the device draw summarised where it lies == the same points handed over, in every entry
    pair = (order[0], order[-1])
    torch.manual_seed(17)
    lying = solver.posterior_summary(n=n, pairs=[pair], quantiles=[0.5], truth=truth)
    torch.manual_seed(17)
    drawn = solver.posterior_collect(solver.posterior_launch(n))
    given = solver.posterior_summary(samples=drawn, pairs=[pair], quantiles=[0.5], truth=truth)
    assert lying["n"] == given["n"] == n and lying["ess"] == given["ess"] == float(n)
    assert set(lying) == set(given) == {"mean", "cov", "resultant", "pair_cov", "quantiles", "n", "ess", "translation_rmse",
                                        "translation_error", "geodesic"}
    for key in ("mean", "cov", "quantiles", "pair_cov"):
        assert set(lying[key]) == set(given[key]) == (set(order) if key != "pair_cov" else {pair})
        for v in lying[key]:
            assert np.array_equal(lying[key][v], given[key][v]), (key, v)
    assert lying["resultant"] == given["resultant"] and set(lying["resultant"]) == {v for v in order if v.dim == 3}
    for key in ("translation_rmse", "translation_error", "geodesic"):
        assert lying[key] == given[key]

    host = {v: np.asarray(drawn[v]) for v in order}
    for v in order:
        circ = [bool(c) for c in v.circular_dim_list]
        (m, c, r), = ST.sample_moments(host[v], [list(range(v.dim))], circular=circ, device=DEV)
        assert np.array_equal(given["mean"][v], m) and np.array_equal(given["cov"][v], c)
        if any(circ):
            assert given["resultant"][v] == r[circ.index(True)]
        h64 = host[v].astype(np.float64)
        for k in range(v.dim):
            if circ[k]:
                R = given["resultant"][v]
                assert R >= 0.1
                want, bound = circmean(h64[:, k], high=np.pi, low=-np.pi), (4 * n * U + 8 * U) / R + 4 * U * np.pi
                assert abs(wrap_pi(given["mean"][v][k] - want)) <= bound, (v, k)
            else:
                want, bound = h64[:, k].mean(), 4 * n * U * np.abs(h64[:, k]).max()
                assert abs(given["mean"][v][k] - want) <= bound, (v, k)
            q = given["quantiles"][v][0, k]
            if circ[k]:
                key = wrap_pi(h64[:, k] - given["mean"][v][k])
                want = np.quantile(key, 0.5) + given["mean"][v][k]
                lo, hi, scale = key.min() + given["mean"][v][k], key.max() + given["mean"][v][k], np.pi
            else:
                want, lo, hi, scale = np.quantile(h64[:, k], 0.5), h64[:, k].min(), h64[:, k].max(), 0.0
            s = np.sort(key if circ[k] else h64[:, k])
            assert lo <= q <= hi
            assert abs(q - want) <= 6 * np.spacing(max(abs(s[n // 2 - 1]), abs(s[n // 2]), scale)), (v, k, q, want)
        assert given["quantiles"][v].shape == (1, v.dim)

    # the pair: symmetric, its diagonal blocks the variables' own bits
    a, b = pair
    P = given["pair_cov"][pair]
    assert P.shape == (a.dim + b.dim,) * 2 and np.array_equal(P, P.T)
    assert np.array_equal(P[:a.dim, :a.dim], given["cov"][a]) and np.array_equal(P[a.dim:, a.dim:], given["cov"][b])

    # truth: the run script's formula on the host copy
    graded = [v for v in order if v in truth]
    err = np.array([host[v].astype(np.float64)[:, :2].mean(0) - np.asarray(truth[v], dtype=np.float64)[:2] for v in graded])
    want = float(np.sqrt((err ** 2).sum(1).mean()))
    print("translation rmse", given["translation_rmse"], want, "geodesic", given["geodesic"])
    assert abs(given["translation_rmse"] - want) <= 1e-12 * want
    assert set(given["translation_error"]) == set(graded) and given["geodesic"] >= 0.0
    assert abs(np.sqrt(np.mean(list(given["translation_error"].values()))) - given["translation_rmse"]) <= 1e-12

    # weights
    unit = solver.posterior_summary(samples=drawn, weights=np.ones(n))
    assert unit["ess"] == float(n) and unit["quantiles"] is None
    for v in order:
        assert np.array_equal(unit["mean"][v], given["mean"][v]) and np.array_equal(unit["cov"][v], given["cov"][v])
    diag = solver.posterior_diagnostics(drawn)
    w = np.exp(diag["log_w"] - diag["log_w"].max())
    imp = solver.posterior_summary(samples=drawn, weights="importance", pairs=[pair])
    byhand = solver.posterior_summary(samples=drawn, weights=w, pairs=[pair])
    print("ess", imp["ess"], byhand["ess"], diag["ess"])
    assert abs(imp["ess"] - diag["ess"]) <= 1e-9 * diag["ess"] and abs(byhand["ess"] - diag["ess"]) <= 1e-9 * diag["ess"]
    worst = 0.0
    for v in order:
        h64 = host[v].astype(np.float64)
        circ = [bool(c) for c in v.circular_dim_list]
        _, _, _, s = oracle_moments(host[v], list(range(v.dim)), circ, w)
        scale_m = np.where(circ, np.pi, np.abs(h64).max(axis=0))
        dm, dc = np.abs(imp["mean"][v] - byhand["mean"][v]), np.abs(imp["cov"][v] - byhand["cov"][v])
        worst = max(worst, float((dm / scale_m).max()), float((dc / np.outer(s, s)).max()))
        assert np.all(dm <= 1e-12 * scale_m), (v, imp["mean"][v], byhand["mean"][v])
        assert np.all(dc <= 1e-12 * np.outer(s, s)), (v, imp["cov"][v], byhand["cov"][v])
        if any(circ):
            assert abs(imp["resultant"][v] - byhand["resultant"][v]) <= 1e-12
    both = np.hstack([host[pair[0]], host[pair[1]]])
    _, _, _, s = oracle_moments(both, list(range(both.shape[1])), [bool(c) for v in pair for c in v.circular_dim_list], w)
    assert np.all(np.abs(imp["pair_cov"][pair] - byhand["pair_cov"][pair]) <= 1e-12 * np.outer(s, s))
    print("importance against by-hand weights: largest relative deviation", worst)
