"""The MMD permutation test without a GPU: the label contract and its packing, the p-value, threshold and Holm algebra, the
identities the kernel rests on, and every refusal of the binding, the statistics front, the solver and the C entry -- all
before a device is needed.  The float64 numpy oracle and the fixture of tests/test_sample_mmd_perm_gpu.py live here too."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_mmd_cpu import Refuse, _fake_graph_solver, wrap_pi
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- shared with tests/test_sample_mmd_perm_gpu.py ------------------------------------------------------------------------------
def pooled_gram(x, y, xcols, ycols, inv_two_sigma2, scale=None, wrap=None):
    """The block's kernel on the pooled set [x; y] in float64 by direct differences, at the float32 points: [m + n, m + n]."""
    x, y = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
    z = np.concatenate([x[:, xcols], y[:, ycols]], axis=0)
    diff = z[:, None, :] - z[None, :, :]
    if wrap is not None:
        diff = np.where(np.asarray(wrap, dtype=bool)[None, None, :], wrap_pi(diff), diff)
    if scale is not None:
        diff = diff * np.asarray(scale, dtype=np.float64)[None, None, :]
    return np.exp(-inv_two_sigma2 * (diff * diff).sum(-1))


def oracle_perm_sums(K, labels):
    """{Sxx', Syy', Sxy'} [P, 3] of the relabelled pooled set by direct sub-matrix sums: no identity, no subtraction."""
    out = np.empty((labels.shape[0], 3))
    for p, l in enumerate(np.asarray(labels, dtype=bool)):
        out[p] = K[np.ix_(l, l)].sum(), K[np.ix_(~l, ~l)].sum(), K[np.ix_(l, ~l)].sum()
    return out


def estimator_value(sums, m, n, estimator):
    """MMDb, or MMDu2 (also what "mmd" is compared on), from {Sxx, Syy, Sxy}: written out here, not taken from the project."""
    sxx, syy, sxy = sums[..., 0], sums[..., 1], sums[..., 2]
    if estimator == "MMDb":
        return np.sqrt(np.maximum(sxx / m ** 2 + syy / n ** 2 - 2.0 * sxy / (m * n), 0.0))
    return (sxx - m) / (m * (m - 1)) + (syy - n) / (n * (n - 1)) - 2.0 * sxy / (m * n)


def oracle_p_value(obs, null):
    """obs [nb], null [nb, P] -> ((1 + #{null >= obs}) / (1 + P) [nb], the smallest |null - obs|)."""
    return (1.0 + (null >= obs[:, None]).sum(1)) / (1.0 + null.shape[1]), float(np.abs(null - obs[:, None]).min())


M, N, COLS = 130, 200, 26


def fixture():
    """x [130, 26], y [200, 26] float32: the issue's recipe in columns 0..7 (3..4 shifted by 0.9, 5 a uniform heading, 6
    headings either side of the seam), and Gaussian columns 8..25 for the wide blocks."""
    rng = np.random.RandomState(21)
    m, n, c = M, N, 8
    x = rng.standard_normal((m, c)) * 1.5 + 3.0
    y = rng.standard_normal((n, c)) * 1.5 + 3.0
    y[:, 3:5] += 0.9
    x[:, 5] = rng.uniform(-np.pi, np.pi, m)
    y[:, 5] = rng.uniform(-np.pi, np.pi, n)
    x[:, 6] = ((rng.standard_normal(m) * 0.3 + 3.1) + np.pi) % (2 * np.pi) - np.pi
    y[:, 6] = ((rng.standard_normal(n) * 0.3 - 3.1) + np.pi) % (2 * np.pi) - np.pi
    wide = np.random.RandomState(22)
    x = np.concatenate([x, wide.standard_normal((m, COLS - c)) * 1.5 + 3.0], axis=1)
    y = np.concatenate([y, wide.standard_normal((n, COLS - c)) * 1.5 + 3.2], axis=1)
    return x.astype(np.float32), y.astype(np.float32)


def table():
    """(xcols, ycols, sigma, scale or None, wrap or None): the issue's seven blocks, then d = 17 across the 16-column chunk,
    a block with a scale, and one whose xcols differ from its ycols."""
    r = lambda a, b: list(range(a, b))                                                        # noqa: E731
    sq = lambda d: float(np.sqrt(d))                                                          # noqa: E731
    rng = np.random.RandomState(23)
    return [
        ([0], [0], 1.0, None, None), ([1, 2], [1, 2], sq(2), None, None), ([3, 4], [3, 4], sq(2), None, None),
        (r(0, 5), r(0, 5), sq(5), None, None), ([5], [5], 1.0, None, [1]), ([6], [6], 1.0, None, [1]),
        ([3, 4, 6], [3, 4, 6], 0.5, None, [0, 0, 1]),
        (r(8, 25), r(8, 25), sq(17), None, None),
        ([0, 1, 7], [0, 1, 7], sq(3), list(rng.uniform(0.5, 2.0, 3)), None),
        (r(9, 13), [12, 11, 10, 9], 2.0, None, None),
    ]


def arrays(tab):
    dims = [len(b[0]) for b in tab]
    blocks = nh.pack_mmd_blocks(dims, [b[2] for b in tab])
    xcols = np.concatenate([b[0] for b in tab]).astype(np.int32)
    ycols = np.concatenate([b[1] for b in tab]).astype(np.int32)
    scale = np.concatenate([np.ones(len(b[0])) if b[3] is None else np.asarray(b[3], dtype=np.float64) for b in tab]) \
        if any(b[3] is not None for b in tab) else None
    wrap = np.concatenate([np.zeros(len(b[0]), dtype=np.uint8) if b[4] is None else np.asarray(b[4], dtype=np.uint8)
                           for b in tab]) if any(b[4] is not None for b in tab) else None
    return blocks, xcols, ycols, scale, wrap


def grams(x, y, tab):
    return [pooled_gram(x, y, b[0], b[1], 1.0 / (2.0 * b[2] ** 2), b[3], b[4]) for b in tab]


# ---- the labels -----------------------------------------------------------------------------------------------------------------
def test_permutation_labels_contract():
    L = ST.permutation_labels(3, 4, 4, seed=7)
    assert L.dtype == np.bool_ and L.shape == (4, 7)
    assert [np.flatnonzero(r).tolist() for r in L] == [[0, 5, 6], [0, 2, 6], [0, 2, 4], [1, 4, 6]]     # PCG64(7), drawn in order
    rng = np.random.Generator(np.random.PCG64(5))
    L = ST.permutation_labels(130, 200, 199, seed=5)
    for p in range(199):
        want = np.zeros(330, dtype=bool)
        want[rng.permutation(330)[:130]] = True
        assert np.array_equal(L[p], want), p
    assert np.all(L.sum(1) == 130)
    assert np.array_equal(ST.permutation_labels(130, 200, 50, seed=5), L[:50])      # a prefix: the rows are drawn in order
    for bad in ((0, 4, 3), (3, 0, 3), (3, 4, 0)):
        with pytest.raises(ValueError):
            ST.permutation_labels(*bad, seed=1)


@pytest.mark.parametrize("P", [1, 63, 64, 65])
def test_pack_perm_labels_round_trip(P):
    L = ST.permutation_labels(5, 9, P, seed=P)
    packed = nh.pack_perm_labels(L)
    assert packed.dtype == np.uint64 and packed.shape == (14, (P + 63) // 64) and packed.flags["C_CONTIGUOUS"]
    for q in range(14):
        for p in range(P):
            assert bool((int(packed[q, p >> 6]) >> (p & 63)) & 1) == bool(L[p, q])
    if P % 64:
        assert np.all(packed[:, -1] >> np.uint64(P % 64) == 0)                      # nothing past the last permutation
    assert np.array_equal(nh.unpack_perm_labels(packed, P), L)
    nh.check_perm_labels(packed, 5, 9, P)
    nh.check_perm_labels(L, 5, 9, P)


def test_check_perm_labels_refusals():
    L = ST.permutation_labels(5, 9, 70, seed=1)
    packed = nh.pack_perm_labels(L)
    for bad, match in ((L.astype(np.uint8), "bool"), (L[:, :13], "permutations, m"), (L[:69], "permutations, m"), (L[0], "bool"),
                       (L.tolist(), "numpy"), (packed[:, :1], "words"), (packed[:13], "words"), (packed.view(np.int64), "bool")):
        with pytest.raises(ValueError, match=match):
            nh.check_perm_labels(bad, 5, 9, 70)
    flipped = L.copy()
    flipped[69, np.flatnonzero(~flipped[69])[0]] = True
    with pytest.raises(ValueError, match="permutation 69 labels 6"):
        nh.check_perm_labels(flipped, 5, 9, 70)
    with pytest.raises(ValueError, match="permutation 69 labels 6"):
        nh.check_perm_labels(nh.pack_perm_labels(flipped), 5, 9, 70)
    stray = packed.copy()
    stray[0, 1] |= np.uint64(1) << np.uint64(40)                                    # a bit past n_perms is ignored
    nh.check_perm_labels(stray, 5, 9, 70)
    with pytest.raises(ValueError, match="not m = 9"):
        nh.check_perm_labels(L, 9, 5, 70)
    with pytest.raises(ValueError, match="at least one permutation"):
        nh.check_perm_labels(L[:0], 5, 9, 0)
    with pytest.raises(ValueError, match="at least one point"):
        nh.check_perm_labels(L, 0, 14, 70)
    with pytest.raises(ValueError, match="bool"):
        nh.pack_perm_labels(L.astype(np.int32))


# ---- the algebra ----------------------------------------------------------------------------------------------------------------
def test_permutation_p_value_and_the_mmd_rule():
    null = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.5, 0.5, 0.5]])
    assert np.array_equal(ST.permutation_p_value([0.3, 0.5], null), [3 / 5, 5 / 5])   # ties count: >=
    assert np.array_equal(ST.permutation_p_value([0.45, 0.6], null), [1 / 5, 1 / 5])  # never 0
    assert np.array_equal(ST.permutation_p_value([0.0], [[1.0]]), [1.0])
    with pytest.raises(ValueError, match="NaN"):
        ST.permutation_p_value([np.nan], [[1.0]])
    with pytest.raises(ValueError, match="at least one value"):
        ST.permutation_p_value([1.0], np.zeros((1, 0)))
    # "mmd" is sqrt(MMDu2), NaN below zero: the test is made on MMDu2.  Sums with m = n = 2 whose MMDu2 are -0.5, -0.25, 0.5 (null)
    # and -0.25 / 0.5 (observed): as square roots NaN, NaN, 0.707 and NaN / 0.707
    def sums_of(u2):
        return np.array([2.0 + 2.0 * 0.5, 2.0 + 2.0 * 0.5, 4.0 * (1.0 - u2) / 2.0])

    null_sums = np.stack([sums_of(v) for v in (-0.5, -0.25, 0.5)])[None]
    for obs_u2, want_p in ((-0.25, 3 / 4), (0.5, 2 / 4), (0.75, 1 / 4)):
        res = ST.permutation_test_from_sums(sums_of(obs_u2)[None], null_sums, 2, 2, "mmd")
        assert res["p_value"][0] == want_p, (obs_u2, res)
        assert np.isnan(res["null"][0, 0]) and np.isnan(res["null"][0, 1]) and abs(res["null"][0, 2] - np.sqrt(0.5)) < 1e-15
        assert np.isnan(res["statistic"][0]) == (obs_u2 < 0)
        same = ST.permutation_test_from_sums(sums_of(obs_u2)[None], null_sums, 2, 2, "MMDu2")
        assert same["p_value"][0] == want_p and abs(same["statistic"][0] - obs_u2) < 1e-15


def test_threshold_is_the_quantile_with_the_observed_value_included():
    null = np.arange(1.0, 20.0)[None]                                              # 19 values, 20 with the observed one
    thr = ST.permutation_threshold([0.0], null, alpha=0.05)                         # the 19th of 20: one value may exceed it
    assert thr[0] == 18.0
    assert ST.permutation_p_value([18.5], null)[0] == 2 / 20 and ST.permutation_p_value([19.5], null)[0] == 1 / 20
    assert ST.permutation_threshold([100.0], null, alpha=0.05)[0] == 19.0
    assert ST.permutation_threshold([0.0], null, alpha=0.5)[0] == 9.0
    with pytest.raises(ValueError, match="alpha"):
        ST.permutation_threshold([0.0], null, alpha=0.0)


def test_holm_adjust_on_a_hand_example():
    # sorted 0.01, 0.02, 0.03, 0.2 -> 4 * 0.01, 3 * 0.02, 2 * 0.03, 1 * 0.2, made monotone
    got = ST.holm_adjust([0.03, 0.01, 0.2, 0.02])
    np.testing.assert_allclose(got, [0.06, 0.04, 0.2, 0.06], rtol=0, atol=1e-16)
    np.testing.assert_allclose(ST.holm_adjust([0.5, 0.4, 0.9]), [1.0, 1.0, 1.0])   # capped at 1
    np.testing.assert_allclose(ST.holm_adjust([0.04]), [0.04])
    np.testing.assert_allclose(ST.holm_adjust([0.01, 0.01]), [0.02, 0.02])
    assert ST.holm_adjust([]).shape == (0,)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        ST.holm_adjust([0.5, 1.5])


def test_the_identities_against_direct_sub_matrix_sums():
    """Sxx' = l' K l, Sxy' = l' t - Sxx', Syy' = T - 2 l' t + Sxx' with t = K 1, T = 1' K 1; the identity labelling gives the
    three sums of the two sets as they are; the upper triangle with the off-diagonal part twice is the whole."""
    x, y = fixture()
    tab = table()
    L = ST.permutation_labels(M, N, 12, seed=5)
    ident = np.zeros((1, M + N), dtype=bool)
    ident[0, :M] = True
    from test_sample_mmd_cpu import oracle_sums
    for b, K in zip(tab, grams(x, y, tab)):
        t, T = K.sum(1), K.sum()
        direct = oracle_perm_sums(K, L)
        lf = L.astype(np.float64)
        sxx = np.einsum("pi,ij,pj->p", lf, K, lf)
        lt = lf @ t
        np.testing.assert_allclose(np.stack([sxx, T - 2.0 * lt + sxx, lt - sxx], 1), direct, rtol=0, atol=1e-12 * T)
        upper = np.triu(K, 1)
        np.testing.assert_allclose(np.einsum("pi,ij,pj->p", lf, upper, lf) * 2.0 + lf.sum(1), sxx, rtol=0, atol=1e-12 * T)
        np.testing.assert_allclose(oracle_perm_sums(K, ident)[0], oracle_sums(x, y, b[0], b[1], 1.0 / (2.0 * b[2] ** 2), b[3], b[4]),
                                   rtol=1e-13)


def test_the_fixture_oracle_p_values_are_the_recorded_ones():
    """The float64 oracle on the fixture, P = 199, seed 5: the p-values the GPU test must reproduce exactly, and the gap
    between the observed value and the nearest null value that makes "exactly" a fair demand."""
    x, y = fixture()
    tab = table()[:7]
    L = ST.permutation_labels(M, N, 199, seed=5)
    ident = np.zeros((1, M + N), dtype=bool)
    ident[0, :M] = True
    Ks = grams(x, y, tab)
    null = np.stack([oracle_perm_sums(K, L) for K in Ks])
    obs = np.stack([oracle_perm_sums(K, ident)[0] for K in Ks])
    p, gap = oracle_p_value(estimator_value(obs, M, N, "MMDb"), estimator_value(null, M, N, "MMDb"))
    np.testing.assert_allclose(p, [0.795, 0.295, 0.005, 0.005, 0.375, 0.045, 0.005], rtol=0, atol=1e-12)
    assert gap >= 1e-7
    p, gap = oracle_p_value(estimator_value(obs, M, N, "MMDu2"), estimator_value(null, M, N, "MMDu2"))
    np.testing.assert_allclose(p, [0.800, 0.295, 0.005, 0.005, 0.375, 0.045, 0.005], rtol=0, atol=1e-12)
    assert gap >= 1e-7
    res = ST.permutation_test_from_sums(obs, null, M, N, "MMDb")
    assert np.array_equal(res["p_value"], oracle_p_value(estimator_value(obs, M, N, "MMDb"), estimator_value(null, M, N, "MMDb"))[0])
    np.testing.assert_allclose(res["p_holm"][[2, 3, 6]], 0.035, rtol=0, atol=1e-12)


# ---- refusals before a device is needed -----------------------------------------------------------------------------------------
def test_the_binding_refuses_before_any_copy(monkeypatch):
    refuse = Refuse()
    for name in ("upload", "_columns"):
        monkeypatch.setattr(nh, name, refuse)
    t = nh.pack_mmd_blocks([2], [1.0])
    X, Y = np.zeros((5, 3), dtype=np.float32), np.zeros((6, 3), dtype=np.float32)
    L = ST.permutation_labels(5, 6, 10, seed=0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.mmd_perm_sums(torch.zeros(5, 3), torch.zeros(6, 3), t, [0, 1], [0, 1], L)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.mmd_perm_sums(X, Y, t, [0, 1], [0, 1], L, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.mmd_perm_sums_t(torch.zeros(3, 5), torch.zeros(3, 6), t, [0, 1], [0, 1], L)
    with pytest.raises(ValueError, match="xcols"):
        nh.mmd_perm_sums(X, Y, t, [0, 3], [0, 1], L, device="cuda")
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        nh.mmd_perm_sums(X[0], Y, t, [0, 1], [0, 1], L, device="cuda")
    with pytest.raises(ValueError, match="permutations, m"):
        nh.mmd_perm_sums(X, Y, t, [0, 1], [0, 1], L[:, :10], device="cuda")
    with pytest.raises(ValueError, match="not m = 6"):
        nh.mmd_perm_sums(Y, X, t, [0, 1], [0, 1], L, device="cuda")
    with pytest.raises(ValueError, match="n_perms"):
        nh.mmd_perm_sums(X, Y, t, [0, 1], [0, 1], nh.pack_perm_labels(L), device="cuda")       # the packed form needs its count
    with pytest.raises(ValueError, match="n_perms"):
        nh.mmd_perm_sums(X, Y, t, [0, 1], [0, 1], L, device="cuda", n_perms=9)
    with pytest.raises(ValueError, match="words"):
        nh.mmd_perm_sums(X, Y, t, [0, 1], [0, 1], nh.pack_perm_labels(L), device="cuda", n_perms=65)
    with pytest.raises(ValueError, match="scale"):
        nh.mmd_perm_sums(X, Y, t, [0, 1], [0, 1], L, scale=np.ones(3), device="cuda")
    assert refuse.calls == 0


def test_mmd_permutation_test_refuses_before_any_copy(monkeypatch):
    refuse = Refuse()
    for name in ("upload", "_columns", "mmd_sums", "mmd_perm_sums"):
        monkeypatch.setattr(nh, name, refuse)
    x, y = np.zeros((5, 3), dtype=np.float32), np.zeros((6, 3), dtype=np.float32)
    for kwargs, match in ((dict(estimator="mmdb"), "estimator"), (dict(permutations=0), "permutations"), (dict(alpha=1.0), "alpha"),
                          (dict(sigma=[1.0, 2.0]), "sigma"), (dict(scale=np.ones(2)), "scale"), (dict(circular=[True]), "circular"),
                          (dict(labels=np.ones((4, 11), dtype=bool)), "not m = 5"),
                          (dict(labels=np.ones((4, 11))), "bool"),
                          (dict(labels=ST.permutation_labels(5, 6, 4, 0)[:, :10]), "permutations, m")):
        with pytest.raises(ValueError, match=match):
            ST.mmd_permutation_test(x, y, [[0, 1]], **kwargs)
    with pytest.raises(ValueError, match="outside"):
        ST.mmd_permutation_test(x, y, [[0, 3]])
    with pytest.raises(ValueError, match="at least 2"):
        ST.mmd_permutation_test(x[:1], y, [[0]], estimator="MMDu2")
    with pytest.raises(ValueError, match="no blocks"):
        ST.mmd_permutation_test(x, y, [])
    assert refuse.calls == 0


def test_posterior_mmd_test_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_mmd_test is NFiSAM.posterior_mmd_test
    nh.build()
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().posterior_mmd_test({})
    s, X0, L1, refuse = _fake_graph_solver(monkeypatch)
    monkeypatch.setattr(nh, "mmd_perm_sums_t", refuse)
    ref = {X0: np.zeros((9, 3)), L1: np.zeros((9, 2))}
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):
        s.posterior_mmd_test(ref)
    for kwargs, match in ((dict(permutations=0), "permutations must be >= 1"), (dict(alpha=0.0), "alpha"), (dict(alpha=1.5), "alpha"),
                          (dict(estimator="nope"), "estimator"), (dict(columns="z"), "columns"), (dict(sigma=-1.0), "sigma"),
                          (dict(variables=[]), "no variable"), (dict(blocks=[()]), "block")):
        with pytest.raises(ValueError, match="posterior_mmd_test: .*" + match):
            s.posterior_mmd_test(ref, own, **kwargs)
    with pytest.raises(ValueError, match="reference lacks variable L1"):
        s.posterior_mmd_test({X0: ref[X0]}, own, variables=[X0, L1])
    with pytest.raises(ValueError, match="at least 2 points"):
        s.posterior_mmd_test({X0: ref[X0][:1], L1: ref[L1][:1]}, own)
    assert refuse.calls == 0


def test_library_exports_the_entries_and_the_c_entry_refuses_on_the_host():
    """The scratch count is two doubles per (block, strip of 64 pooled points, permutation rounded up to 256) and one per
    (block, strip), 0 for what the entry refuses; the entry refuses on the host, before it touches the device (the pointers
    below are never dereferenced: they are not device memory)."""
    nh.build()
    lib = nh.lib()
    for name in ("nfisam_sample_mmd_perm", "nfisam_sample_mmd_perm_scratch_count"):
        assert name in nh.EXPORTS and hasattr(lib, name), name
    assert lib.nfisam_abi_version() == 1600
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    assert "int nfisam_sample_mmd_perm(" in hdr and "size_t nfisam_sample_mmd_perm_scratch_count(" in hdr
    assert "#define NFISAM_MMD_PERM_MAX %d" % nh.MMD_PERM_MAX in hdr
    count = lib.nfisam_sample_mmd_perm_scratch_count
    assert count(1, 1, 1, 1) == 2 * (2 * 256 + 1) and count(64, 64, 3, 256) == 3 * 2 * (2 * 256 + 1)
    assert count(65, 64, 1, 257) == 3 * (2 * 512 + 1) and count(130, 200, 7, 199) == 7 * 7 * (2 * 256 + 1)
    assert count(0, 5, 1, 1) == 0 and count(5, 0, 1, 1) == 0 and count(5, 5, 0, 1) == 0 and count(5, 5, 65536, 1) == 0
    assert count(5, 5, 1, 0) == 0 and count(5, 5, 1, -3) == 0 and count(5, 5, 1, nh.MMD_PERM_MAX + 1) == 0
    assert count(5, 5, 1, nh.MMD_PERM_MAX) == 2 * (2 * nh.MMD_PERM_MAX + 1)
    assert count(64 * 4000, 64 * 4000, 65535, 256) == 0                             # more groups than a launch holds
    blocks = nh.pack_mmd_blocks([2], [1.0])
    fake = C.c_void_p(4096)

    def call(Xt=fake, m=5, n=5, blk=blocks, nb=1, labels=fake, perms=10, sums=fake):
        return lib.nfisam_sample_mmd_perm(Xt, 4, m, fake, 4, n, blk.ctypes.data_as(C.c_void_p), fake, nb, fake, fake, 2, None, None,
                                          labels, perms, sums, fake, None)
    assert call(labels=None) == nh.ERR_ARG and call(perms=0) == nh.ERR_ARG and call(perms=-1) == nh.ERR_ARG
    assert call(perms=nh.MMD_PERM_MAX + 1) == nh.ERR_ARG
    assert call(Xt=None) == nh.ERR_ARG and call(sums=None) == nh.ERR_ARG
    assert call(m=0) == nh.ERR_ARG and call(n=0) == nh.ERR_ARG and call(nb=0) == nh.ERR_ARG and call(nb=65536) == nh.ERR_ARG
    for d, v in ((0, 0.5), (2, 0.0), (2, -1.0), (2, np.inf), (2, np.nan)):
        bad = blocks.copy()
        bad["d"], bad["inv_two_sigma2"] = d, v
        assert call(blk=bad) == nh.ERR_ARG, (d, v)
