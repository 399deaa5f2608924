"""The kernel Stein discrepancy without a GPU: a float64 numpy restatement of the Stein sums of `nfisam_sample_ksd` (kept
here; the GPU tests use it for the shapes the fixture lacks and for wrapped columns) against the reference's own
`Gaussian_kernel_stein_discrepancy` stored in tests/golden/factor_score.npz part (c), `ksd_from_sums`, and every refusal of
the new bindings and of `utils.Statistics` before anything is launched.

Bound of the restatement against the fixture: |ours - ref| <= TOL_C (|ref| + 1) with TOL_C = 16 x 5.2e-14, the largest
deviation measured over off_ksd (5.13e-14: h_ij is a difference of the four terms p1 .. p4, each up to 1e3 x the result),
ustats and vstats (both 0: the sums agree to the bit); both sides are float64 sums of the same 13 products per pair, the
reference's through D x D matrix products."""
import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_factor_score_cpu import deviation, score_fixture
from utils import Statistics as ST

MEASURED_C = 5.2e-14
TOL_C = 16 * MEASURED_C


# ---- shared with tests/test_sample_ksd_gpu.py --------------------------------------------------------------------------------
def stein_matrix(x, score, precision, wrap=None):
    """H [n, n] float64 at the float32 points: h_ij = k_ij [s_i.s_j + sum (s_i - s_j) p d - sum p^2 d^2 + sum p], d = x_i - x_j
    brought into [-pi, pi] as sign(d) wrap(|d|) in the columns flagged by `wrap`, k_ij = exp(-sum p d^2 / 2)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    s, p = np.asarray(score, dtype=np.float64), np.asarray(precision, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    if wrap is not None:
        m = (np.abs(d) + np.pi) % (2.0 * np.pi) - np.pi
        d = np.where(np.asarray(wrap, dtype=bool)[None, None, :], np.sign(d) * m, d)
    pd = p * d
    k = np.exp(-0.5 * (pd * d).sum(-1))
    return k * (s @ s.T + ((s[:, None, :] - s[None, :, :]) * pd).sum(-1) - (pd * pd).sum(-1) + p.sum())


def stein_stats(H):
    n = H.shape[0]
    return ST.ksd_from_sums(H.sum(), np.trace(H), n, ustat=n >= 2)


def bootstrap(off, draws):
    n = off.shape[0]
    return np.array([(w / n - 1.0 / n) @ off @ (w / n - 1.0 / n) for w in np.asarray(draws, dtype=np.float64)])


# ---- the restatement against the reference ----------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_run():
    fs = score_fixture()
    x, s, p = fs["ksd_samples"], fs["ksd_score"], fs["ksd_precision"]
    assert x.shape == s.shape == (130, 13) and x.dtype == np.float32 and p.shape == (13,)
    H = stein_matrix(x, s, p)
    off = H - np.diag(np.diag(H))
    u, v = stein_stats(H)
    d_off, d_u, d_v = deviation(off, fs["ksd_off"]), deviation(u, fs["ksd_ustats"]), deviation(v, fs["ksd_vstats"])
    print("|ours - ref| / (|ref| + 1): off_ksd %.3g, ustats %.3g, vstats %.3g" % (d_off, d_u, d_v))
    assert max(d_off, d_u, d_v) <= TOL_C
    assert np.allclose(np.diag(H), (s * s).sum(1) + p.sum(), rtol=1e-14, atol=0.0)
    assert np.array_equal(H, H.T)
    boot = bootstrap(fs["ksd_off"], fs["ksd_draws"])
    assert float(np.mean(boot >= float(fs["ksd_ustats"]))) == float(fs["ksd_p_u"])
    assert float(np.mean(bootstrap(off, fs["ksd_draws"]) >= u)) == float(fs["ksd_p_u"])


def test_wrapped_differences_are_antisymmetric_and_continuous_across_the_seam():
    x = np.array([[3.1], [-3.1], [0.2]], dtype=np.float32)
    s = np.array([[0.5], [-1.0], [2.0]])
    H = stein_matrix(x, s, [0.7], wrap=[1])
    assert np.array_equal(H, H.T)
    d = 2 * np.pi - (float(x[0, 0]) - float(x[1, 0]))                 # the short way round, from -3.1 up to 3.1
    want = np.exp(-0.35 * d * d) * (0.5 * -1.0 + (0.5 + 1.0) * 0.7 * -d - 0.49 * d * d + 0.7)
    assert np.isclose(H[0, 1], want, rtol=1e-12, atol=0.0)
    assert not np.isclose(stein_matrix(x, s, [0.7])[0, 1], want, rtol=1e-3, atol=0.0)


def test_ksd_from_sums():
    u, v = ST.ksd_from_sums(30.0, 6.0, 4)
    assert u == 24.0 / 12.0 and v == 30.0 / 16.0
    assert ST.ksd_from_sums(5.0, 5.0, 1, ustat=False) == (None, 5.0)
    with pytest.raises(ValueError, match="at least two points"):
        ST.ksd_from_sums(5.0, 5.0, 1)
    with pytest.raises(ValueError, match="at least one point"):
        ST.ksd_from_sums(0.0, 0.0, 0, ustat=False)


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
def test_ksd_binding_refuses_bad_input_with_no_device():
    X, G, p = np.zeros((5, 3), dtype=np.float32), np.zeros((5, 3)), np.ones(3)
    with pytest.raises(ValueError, match="shape of the points"):
        nh.ksd_sums(X, G[:, :2], p, device="cuda")
    with pytest.raises(ValueError, match="shape of the points"):
        nh.ksd_sums(X, G[:4], p, device="cuda")
    with pytest.raises(ValueError, match="one value per column"):
        nh.ksd_sums(X, G, np.ones(2), device="cuda")
    with pytest.raises(ValueError, match="one value per column"):
        nh.ksd_sums(X, G, np.eye(3), device="cuda")
    for bad in (np.array([1.0, -1e-9, 1.0]), np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0])):
        with pytest.raises(ValueError, match="finite and >= 0"):
            nh.ksd_sums(X, G, bad, device="cuda")
    with pytest.raises(ValueError, match="one flag per column"):
        nh.ksd_sums(X, G, p, wrap=[1, 0], device="cuda")
    with pytest.raises(ValueError, match="at least one point"):
        nh.ksd_sums(X[:0], G[:0], p, device="cuda")
    with pytest.raises(ValueError, match="tensors or arrays"):
        nh.ksd_sums(X[0], G[0], p, device="cuda")
    big = np.zeros((nh.KSD_MATRIX_MAX_N + 1, 1), dtype=np.float32)
    with pytest.raises(ValueError, match="at most 4096 points"):
        nh.ksd_sums(big, big.astype(np.float64), np.ones(1), matrix=True, device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.ksd_sums(X, G, p, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.ksd_sums_t(torch.zeros(3, 5), torch.zeros(3, 5, dtype=torch.float64), p)


def test_statistics_refuse_bad_input_with_no_device():
    x, s = np.zeros((6, 3), dtype=np.float32), np.zeros((6, 3))
    with pytest.raises(ValueError, match="shape of x"):
        ST.kernel_stein_discrepancy(x, s[:, :2])
    with pytest.raises(ValueError, match="points, columns"):
        ST.kernel_stein_discrepancy(x[0], s[0])
    with pytest.raises(ValueError, match="sigma must be positive"):
        ST.kernel_stein_discrepancy(x, s, sigma=0.0)
    with pytest.raises(ValueError, match="one value per column"):
        ST.kernel_stein_discrepancy(x, s, scale=np.ones(2))
    with pytest.raises(ValueError, match="scale must be finite"):
        ST.kernel_stein_discrepancy(x, s, scale=np.array([1.0, np.nan, 1.0]))
    with pytest.raises(ValueError, match="one flag per column"):
        ST.kernel_stein_discrepancy(x, s, circular=[True])
    with pytest.raises(ValueError, match="nboot"):
        ST.kernel_stein_discrepancy(x, s, nboot=-1)
    with pytest.raises(ValueError, match="at least two points"):
        ST.kernel_stein_discrepancy(x[:1], s[:1], nboot=3)
    with pytest.raises(ValueError, match="at most 4096 points"):
        ST.kernel_stein_discrepancy(np.zeros((4097, 1), dtype=np.float32), np.zeros((4097, 1)), matrix=True, device="cuda")
    # the reference's name: a [D] vector or a diagonal [D, D] matrix; any other dense matrix is refused, saying so
    dense = np.eye(3)
    dense[0, 2] = 1e-3
    with pytest.raises(ValueError, match="off-diagonal"):
        ST.Gaussian_kernel_stein_discrepancy(s, dense, x)
    with pytest.raises(ValueError, match="vector or a diagonal"):
        ST.Gaussian_kernel_stein_discrepancy(s, np.ones(2), x)
    with pytest.raises(ValueError, match="finite and >= 0"):
        ST.Gaussian_kernel_stein_discrepancy(s, -np.eye(3), x)
    with pytest.raises(ValueError, match="at least two points"):
        ST.Gaussian_kernel_stein_discrepancy(s[:1], np.eye(3), x[:1])
    with pytest.raises(ValueError, match="shape of samples"):
        ST.Gaussian_kernel_stein_discrepancy(s[:, :2], np.eye(3), x)
    with pytest.raises(ValueError, match="nboot"):
        ST.Gaussian_kernel_stein_discrepancy(s, np.eye(3), x, nboot=0)
    assert np.array_equal(ST._diagonal_precision(np.diag([1.0, 0.0, 2.5]), 3), [1.0, 0.0, 2.5])      # the diagonal form
    assert np.array_equal(ST._diagonal_precision([1.0, 0.0, 2.5], 3), [1.0, 0.0, 2.5])


def test_solver_methods_refuse_before_a_graph_exists():
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    solver = NFiSAM(NFiSAMArgs())
    with pytest.raises(RuntimeError, match="no factor graph yet"):
        solver.joint_score({})
    with pytest.raises(RuntimeError, match="no factor graph yet"):
        solver.posterior_ksd()
