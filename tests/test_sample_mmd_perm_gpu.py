"""The MMD permutation test on the GPU (nfisam_sample_mmd_perm through nfisam_hip.mmd_perm_sums,
utils.Statistics.mmd_permutation_test and NFiSAM.posterior_mmd_test).

The oracle is a float64 numpy evaluation by direct differences on the relabelled pooled set (`pooled_gram` and
`oracle_perm_sums` of tests/test_sample_mmd_perm_cpu.py: plain sub-matrix sums, none of the kernel's identities).  Bound per
sum: |S_dev - S_ref| <= 4e-11 T_ref, T_ref the block's pooled total 1' K 1.  Each output is a signed combination of at most
four sums of positive terms, each <= T, and each of those carries the 1e-11 relative bound of the error analysis in
tests/test_sample_mmd_gpu.py (positive terms, float64 chain).  The bound is relative to T, not to the sum itself: a
legitimately tiny Sxy' is not held to digits a subtraction cannot give.

The p-values are compared EXACTLY: the oracle's smallest |null - observed| is asserted to be >= 1e-7, while the rounding of an
MMD^2 value at these sizes is at most 4e-11 (N^2 / (m n))^2 ~ 7e-10."""
import json
import os

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_mmd_perm_cpu import (M, N, arrays, estimator_value, fixture, grams, oracle_p_value, oracle_perm_sums,
                                      pooled_gram, table)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
BOUND = 4e-11
_cache = {}


def _grams(m, n):
    """The ten pooled Gram matrices of the fixture's first m and n points: computed once per shape and shared, never changed."""
    if (m, n) not in _cache:
        x, y = fixture()
        _cache[(m, n)] = grams(x[:m], y[:n], table())
    return _cache[(m, n)]


def _identity(m, n):
    ident = np.zeros((1, m + n), dtype=bool)
    ident[0, :m] = True
    return ident


def _ratio(dev, ref, Ks):
    """max |dev - ref| / (BOUND T) over blocks, permutations and sums: <= 1 inside the bound."""
    T = np.array([K.sum() for K in Ks])
    return float(np.max(np.abs(dev - ref) / (BOUND * T[:, None, None])))


@pytest.mark.parametrize("m,n,P", [(1, 64, 1), (1, 64, 65), (63, 65, 63), (64, 64, 64), (64, 64, 199), (65, 200, 65), (65, 200, 1),
                                   (130, 200, 199), (130, 200, 63)])
def test_sums_match_the_float64_oracle(m, n, P):
    """All ten blocks in one table around the 64-point tile and the 64-permutation word.  Largest |dev - ref| / T measured on
    the MI355X over the nine cases: 5.0e-16; the bound stays the 4e-11 of the error analysis."""
    x, y = fixture()
    x, y = x[:m], y[:n]
    Ks = _grams(m, n)
    L = ST.permutation_labels(m, n, P, seed=5)
    dev = nh.mmd_perm_sums(x, y, *arrays(table())[:3], L, *arrays(table())[3:], device=DEV).cpu().numpy()
    ref = np.stack([oracle_perm_sums(K, L) for K in Ks])
    assert dev.shape == (10, P, 3) and dev.dtype == np.float64
    ratio = _ratio(dev, ref, Ks)
    print("m %d n %d P %d: largest |dev - ref| / T %.3g (bound %.1g)" % (m, n, P, ratio * BOUND, BOUND))
    assert np.all(np.isfinite(dev)) and ratio <= 1.0, (ratio, dev[:, 0], ref[:, 0])


def test_the_identity_labelling_reproduces_mmd_sums():
    x, y = fixture()
    blocks, xcols, ycols, scale, wrap = arrays(table())
    Ks = _grams(M, N)
    for m, n in ((M, N), (64, 64), (1, 64)):
        want = nh.mmd_sums(x[:m], y[:n], blocks, xcols, ycols, scale, wrap, device=DEV).cpu().numpy()
        got = nh.mmd_perm_sums(x[:m], y[:n], blocks, xcols, ycols, _identity(m, n), scale, wrap, device=DEV).cpu().numpy()
        ratio = _ratio(got, want[:, None, :], _grams(m, n))
        print("identity labelling m %d n %d: largest |perm - mmd_sums| / T %.3g" % (m, n, ratio * BOUND))
        assert got.shape == (10, 1, 3) and ratio <= 1.0, (got[:, 0], want)
    assert Ks is _grams(M, N)


def test_second_call_block_position_permutation_position_and_chunking_give_the_same_bits():
    x, y = fixture()
    tab = table()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    L = ST.permutation_labels(M, N, 199, seed=5)

    def run(t, labels, **kw):
        b, xc, yc, sc, wr = arrays(t)
        return nh.mmd_perm_sums(xd, yd, b, xc, yc, labels, sc, wr, **kw)

    first = run(tab, L)
    assert torch.equal(run(tab, L), first)                                          # the same call twice
    assert torch.equal(run(tab[::-1], L).flip(0), first)                            # every block at another position
    for k in (0, 5, 7, 8, 9):                                                       # alone: also without the others' scale / wrap
        assert torch.equal(run([tab[k]], L)[0], first[k]), k
    assert torch.equal(run([tab[3], tab[6], tab[3]], L), first[[3, 6, 3]])
    assert torch.equal(run(tab, L[70:71])[:, 0], first[:, 70])                      # permutation 70 alone
    assert torch.equal(run(tab, L[[70, 3, 198]]), first[:, [70, 3, 198]])           # and first of three
    # P = 130 in one call against chunks of 64 + 66, and the packed form against the bool one
    whole = run(tab, L[:130])
    assert torch.equal(whole, first[:, :130])
    assert torch.equal(torch.cat([run(tab, L[:64]), run(tab, L[64:130])], dim=1), whole)
    assert torch.equal(run(tab, nh.pack_perm_labels(L), n_perms=199), first)
    # the column-major twin uses the matrices in place
    b, xc, yc, sc, wr = arrays(tab)
    twin = nh.mmd_perm_sums_t(xd.t().contiguous(), yd.t().contiguous(), b, xc, yc, L, sc, wr)
    assert torch.equal(twin, first)


def test_the_binding_splits_long_calls_at_its_scratch_budget(monkeypatch):
    """600 permutations with the budget shrunk to one 256-permutation launch: three launches, the same bits as one."""
    x, y = fixture()
    b, xc, yc, sc, wr = arrays(table()[:3])
    L = ST.permutation_labels(M, N, 600, seed=9)
    whole = nh.mmd_perm_sums(x, y, b, xc, yc, L, sc, wr, device=DEV)
    monkeypatch.setattr(nh, "MMD_PERM_SCRATCH_BYTES", 1)
    split = nh.mmd_perm_sums(x, y, b, xc, yc, L, sc, wr, device=DEV)
    assert whole.shape == (3, 600, 3) and torch.equal(split, whole)
    monkeypatch.setattr(nh, "MMD_PERM_MAX", 256)
    assert torch.equal(nh.mmd_perm_sums(x, y, b, xc, yc, L, sc, wr, device=DEV), whole)


def test_a_bad_block_given_to_the_c_entry_yields_nan_and_leaves_the_others_alone():
    """`checked=True` skips the binding's table check: the C entry sees a row past x_rows and a block past n_entries."""
    x, y = fixture()
    blocks, xcols, ycols, _, _ = arrays(table()[:4])
    L = ST.permutation_labels(M, N, 5, seed=2)
    good = nh.mmd_perm_sums(x, y, blocks, xcols, ycols, L, device=DEV)
    Xt, Yt = torch.from_numpy(x.T.copy()).to(DEV), torch.from_numpy(y.T.copy()).to(DEV)
    bad_x = xcols.copy()
    bad_x[1] = x.shape[1]                                # block 1 = entries 1..2: one row past the matrix
    got = nh.mmd_perm_sums_t(Xt, Yt, blocks, bad_x, ycols, L, checked=True)
    assert torch.isnan(got[1]).all() and torch.equal(got[[0, 2, 3]], good[[0, 2, 3]])
    past = blocks.copy()
    past["col_off"][3] = int(xcols.size) - 2             # d = 5: runs past the lists
    got = nh.mmd_perm_sums_t(Xt, Yt, past, xcols, ycols, L, checked=True)
    assert torch.isnan(got[3]).all() and torch.equal(got[:3], good[:3])
    with pytest.raises(ValueError):
        nh.mmd_perm_sums_t(Xt, Yt, past, xcols, ycols, L)


@pytest.mark.parametrize("estimator", ["MMDb", "MMDu2"])
def test_p_values_equal_the_oracles_exactly(estimator):
    """The issue's seven blocks, P = 199, labels of seed 5: MMDb 0.795 0.295 0.005 0.005 0.375 0.045 0.005, MMDu2 0.800 for the
    first block.  Block [6] is 6.2 rad apart without the wrap and 0.08 rad with it: the wrap of the pooled walk is covered."""
    x, y = fixture()
    x, y = x[:, :8], y[:, :8]
    tab = table()[:7]
    cols = [b[0] for b in tab]
    sigma = [b[2] for b in tab]
    circular = [False] * 5 + [True, True, False]
    L = ST.permutation_labels(M, N, 199, seed=5)
    Ks = _grams(M, N)[:7]
    obs = estimator_value(np.stack([oracle_perm_sums(K, _identity(M, N))[0] for K in Ks]), M, N, estimator)
    null = estimator_value(np.stack([oracle_perm_sums(K, L) for K in Ks]), M, N, estimator)
    want, gap = oracle_p_value(obs, null)
    assert gap >= 1e-7, gap                                                         # the precondition of "exactly"
    res = ST.mmd_permutation_test(x, y, cols, permutations=199, seed=5, estimator=estimator, sigma=sigma, circular=circular,
                                  device=DEV)
    print(estimator, "p", res["p_value"], "oracle", want, "gap", gap)
    assert np.array_equal(res["p_value"], want)
    np.testing.assert_allclose(want, [0.795 if estimator == "MMDb" else 0.8, 0.295, 0.005, 0.005, 0.375, 0.045, 0.005], atol=1e-12)
    stat = ST.mmd_blocks(x, y, cols, estimator=estimator, sigma=sigma, circular=circular, device=DEV)
    assert np.all(res["statistic"] == stat)
    assert res["null"].shape == (7, 199) and np.max(np.abs(res["null"] - null)) <= 1e-8
    assert res["permutations"] == 199 and res["seed"] == 5 and res["estimator"] == estimator and (res["m"], res["n"]) == (M, N)
    assert np.array_equal(res["p_holm"], ST.holm_adjust(want))
    assert np.array_equal(res["threshold"] < res["statistic"], want <= 0.05)        # above the threshold <=> p <= alpha
    given = ST.mmd_permutation_test(x, y, cols, seed=77, estimator=estimator, sigma=sigma, circular=circular, labels=L, device=DEV)
    assert given["seed"] is None and given["permutations"] == 199 and np.array_equal(given["p_value"], want)
    if estimator == "MMDu2":                                                        # "mmd": the same test, made on the MMDu2 values
        root = ST.mmd_permutation_test(x, y, cols, permutations=199, seed=5, estimator="mmd", sigma=sigma, circular=circular,
                                       device=DEV)
        assert np.array_equal(root["p_value"], want)
        assert np.array_equal(np.isnan(root["null"]), res["null"] < 0)


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def _law(v, count, seed, k, shift=0.0):
    """[count, dim] float32 from a generator of (seed, k) alone: spread 0.5 around 2 k (+ shift in x and y), headings uniform."""
    rng = np.random.Generator(np.random.PCG64([seed, k]))
    a = rng.standard_normal((count, v.dim)) * 0.5 + 2.0 * k
    if v.dim == 3:
        a[:, 2] = rng.uniform(-np.pi, np.pi, count)
    a[:, :2] += shift
    return a.astype(np.float32)


def _solver_oracle(own, ref, order, labels, estimator, columns="xy", standardise=False):
    """The p-values of the joint block and of every variable's block, float64 numpy: -> ([1 + variables], smallest gap)."""
    take = (lambda v: v.dim) if columns == "all" else (lambda v: min(v.dim, 2))             # noqa: E731
    x = np.concatenate([own[v][:, :take(v)] for v in order], 1)
    y = np.concatenate([ref[v][:, :take(v)] for v in order], 1)
    circ = np.concatenate([np.asarray(v.circular_dim_list[:take(v)], dtype=bool) for v in order])
    off = np.cumsum([0] + [take(v) for v in order])
    scale = np.ones(x.shape[1])
    if standardise:
        std = np.maximum(np.concatenate([x, y], 0).astype(np.float64).std(0), 1e-3)
        scale = np.where(circ, 1.0, 1.0 / std)
    n, m = x.shape[0], y.shape[0]
    ident = np.zeros((1, n + m), dtype=bool)
    ident[0, :n] = True
    ps, gaps = [], []
    for c in [list(range(x.shape[1]))] + [list(range(off[i], off[i + 1])) for i in range(len(order))]:
        sig = 1.0 if estimator == "mmd" else np.sqrt(len(c))
        K = pooled_gram(x, y, c, c, 1.0 / (2.0 * sig ** 2), scale[c], circ[c])
        kind = "MMDb" if estimator == "MMDb" else "MMDu2"
        p, gap = oracle_p_value(estimator_value(oracle_perm_sums(K, ident), n, m, kind),
                                estimator_value(oracle_perm_sums(K, labels)[None], n, m, kind))
        ps.append(float(p[0]))
        gaps.append(gap)
    return np.array(ps), min(gaps)


def test_posterior_mmd_test_on_the_small_range_graph(tmp_path):
    """The graph of the first two updates of the small range problem (X0, L1, L2, X1), the samples GIVEN -- from seeded numpy
    generators, so nothing depends on a device draw and no flow is trained.  Without `standardise` the values are
    `posterior_mmd`'s; a reference shifted by 5 m is rejected everywhere at the smallest p-value there is; a reference from the
    same law (seed 3: the oracle's joint p-value is 0.415, its marginal ones 0.28, 0.515, 0.71, 0.275 in the order X0, L1, L2,
    X1) is not, and its p-values are the oracle's; `standardise` takes the POOLED spread."""
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
    fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
    kwargs = json.loads(str(fx["arguments"]))
    kwargs["cuda_training"] = True
    path = tmp_path / "factor_graph.fg"
    path.write_text(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    nodes, truth, factors = graph_file_parser(str(path), "fg", prior_cov_scale=0.1)
    steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))[:2]
    solver = NFiSAM(NFiSAMArgs(**kwargs))
    for vs, fs in steps:
        for v in vs: solver.add_node(v)
        for f in fs: solver.add_factor(f)
        solver.update_physical_and_working_graphs()
    order = list(solver.elimination_ordering)
    names = sorted(v.name for v in order)
    assert names == ["L1", "L2", "X0", "X1"]
    P, seed = 199, 3
    own = {v: _law(v, 150, 3, names.index(v.name)) for v in order}
    same = {v: _law(v, 120, 103, names.index(v.name)) for v in order}
    far = {v: _law(v, 120, 103, names.index(v.name), shift=5.0) for v in order}
    labels = ST.permutation_labels(150, 120, P, seed)                               # the posterior points are the first set

    plain = solver.posterior_mmd(same, own)
    res = solver.posterior_mmd_test(same, own, permutations=P, seed=seed)
    for key in ("joint", "marginal", "blocks", "marginal_mean", "floor", "m", "n", "estimator"):
        a, b = res[key], plain[key]
        assert a == b or (key == "marginal" and all(a[v] == b[v] or (np.isnan(a[v]) and np.isnan(b[v])) for v in order)) or \
            (np.isnan(a) and np.isnan(b)), key
    want, gap = _solver_oracle(own, same, order, labels, "mmd")
    print("same law: joint p", res["p_value"]["joint"], "oracle", want, "gap", gap)
    assert gap >= 1e-7
    assert res["p_value"]["joint"] == want[0] == 0.415
    assert [res["p_value"]["marginal"][v] for v in order] == list(want[1:])
    assert res["rejected"] == [] and res["p_value"]["blocks"] == []
    holm = ST.holm_adjust(want[1:])
    assert [res["marginal_p_holm"][v] for v in order] == list(holm)
    assert (res["permutations"], res["seed"], res["alpha"]) == (P, seed, 0.05)
    assert set(res["threshold"]["marginal"]) == set(order)

    shifted = solver.posterior_mmd_test(far, own, permutations=P, seed=seed, blocks=[(order[0], order[-1])])
    assert shifted["p_value"]["joint"] == 1.0 / (P + 1) and shifted["p_value"]["blocks"] == [1.0 / (P + 1)]
    assert all(p == 1.0 / (P + 1) for p in shifted["p_value"]["marginal"].values())
    assert shifted["rejected"] == order
    assert all(abs(p - 4.0 / (P + 1)) < 1e-15 for p in shifted["marginal_p_holm"].values())

    std = solver.posterior_mmd_test(same, own, permutations=P, seed=seed, estimator="MMDb", columns="all", standardise=True)
    want, gap = _solver_oracle(own, same, order, labels, "MMDb", columns="all", standardise=True)
    print("standardised, all columns: joint p", std["p_value"]["joint"], "oracle", want, "gap", gap)
    assert gap >= 1e-7
    assert std["p_value"]["joint"] == want[0] and [std["p_value"]["marginal"][v] for v in order] == list(want[1:])
    # a scale from the reference alone (what posterior_mmd's standardise takes) is another kernel: the observed values differ
    one = solver.posterior_mmd(same, own, estimator="MMDb", columns="all", standardise=True)
    assert one["joint"] != std["joint"]
