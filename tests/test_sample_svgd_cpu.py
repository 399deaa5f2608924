"""The Stein variational direction and step without a GPU: a float64 numpy restatement of `nfisam_sample_svgd` and
`nfisam_sample_step` (kept here; tests/test_sample_svgd_gpu.py grades the device against it), the refinement conditions met by
that arithmetic alone, and every refusal of the new bindings, of `utils.Statistics` and of the solver's two methods before a
device is touched.

The reference has no SVGD: the restatement is the yardstick -- direct pairwise differences, the signed wrap
sign(d) wrap(|d|), the AdaGrad-with-decay step with its rounding to float32.

THE REFINEMENT CONDITIONS.  Target N(mu, diag sigma^2), mu = (40, -7, 3.1), sigma = (0.5, 2.0, 0.2), the third column circular
(the particles straddle +-pi); start mu + (3, 3, 0.6) sigma + 0.3 sigma randn (RandomState(7)); scale = 1 / the start's spread;
bandwidth sqrt(block width); eps = 0.05 in every column; 500 steps.  Conditions, for n in {65, 130}, one joint block and the
blocks {0, 1}, {2}: |mean error| <= 0.1 sigma and 0.6 <= std / sigma <= 1.2 in every column.  Plain ascent, 300 steps: every
particle ends within eps of mu (the AdaGrad step settles into an oscillation of eps / 2 about the mode)."""
import os
import re

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSIDE = np.nextafter(np.float32(np.pi), np.float32(0)) * np.float32(-1)      # the float32 just inside -pi


# ---- shared with tests/test_sample_svgd_gpu.py -------------------------------------------------------------------------------
def signed_wrap(d):
    """sign(d) wrap(|d|): into [-pi, pi], antisymmetric to the bit."""
    return np.sign(d) * ((np.abs(d) + np.pi) % (2.0 * np.pi) - np.pi)


def direction(x, g, table, cols, scale=None, wrap=None):
    """Phi [n_entries, n] float64 at the float32 points x [n, x_cols] with scores g [n, x_cols]: for block b of `table`
    (MMD_BLOCK_DTYPE) and its entries e, d = x_i - x_j in column cols[e] (signed wrap where wrap[e]),
    k = exp(-inv sum_e (scale_e d)^2), Phi[e, i] = sum_j k_ij (g[j, cols[e]] + 2 inv scale_e^2 d_ij) / n."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    g, cols = np.asarray(g, dtype=np.float64), np.asarray(cols)
    nh.check_svgd_blocks(table, cols, x.shape[1], scale, wrap)             # (the yardstick takes what the binding takes)
    n, ne = x.shape[0], cols.size
    sc = np.ones(ne) if scale is None else np.asarray(scale, dtype=np.float64)
    wr = np.zeros(ne, dtype=bool) if wrap is None else np.asarray(wrap, dtype=bool)
    phi = np.zeros((ne, n))
    for row in table:
        e = np.arange(int(row["col_off"]), int(row["col_off"]) + int(row["d"]))
        c, inv = cols[e], float(row["inv_two_sigma2"])
        d = x[:, None, c] - x[None, :, c]                                  # [i, j, entry]
        d = np.where(wr[e][None, None, :], signed_wrap(d), d)
        k = np.exp(-inv * ((sc[e] * d) ** 2).sum(-1))
        phi[e] = ((k[:, :, None] * (g[None, :, c] + 2.0 * inv * sc[e] ** 2 * d)).sum(1) / n).T
    return phi


def step(x, cols, phi, hist, eps, wrap=None, alpha=0.9, fudge=1e-6, first=False):
    """One AdaGrad-with-decay step -> (the new float32 points [n, x_cols], the new hist [n_entries, n])."""
    x, cols = np.array(x, dtype=np.float32), np.asarray(cols)
    phi, eps = np.asarray(phi, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    nh.check_step_args(alpha, fudge, eps)                                  # (the yardstick takes what the binding takes)
    h = phi * phi if first else alpha * np.asarray(hist, dtype=np.float64) + (1.0 - alpha) * (phi * phi)
    for e, c in enumerate(cols):
        y = x[:, c].astype(np.float64) + eps[e] * phi[e] / (np.sqrt(h[e]) + fudge)
        if wrap is not None and wrap[e]:
            y = (y + np.pi) % (2.0 * np.pi) - np.pi
            f = y.astype(np.float32)
            f[~((f.astype(np.float64) < np.pi) & (f.astype(np.float64) >= -np.pi))] = INSIDE
        else:
            f = y.astype(np.float32)
        x[:, c] = f
    return x, h


def refine(x, score, table, cols, eps, steps, scale=None, wrap=None, kernel=True, alpha=0.9, fudge=1e-6):
    """`steps` times direction (or, without `kernel`, the score itself) + step -> the refined float32 points."""
    x, hist = np.array(x, dtype=np.float32), None
    for t in range(steps):
        g = score(x.astype(np.float64))
        phi = direction(x, g, table, cols, scale, wrap) if kernel else np.ascontiguousarray(g[:, np.asarray(cols)].T)
        x, hist = step(x, cols, phi, hist, eps, wrap, alpha, fudge, first=t == 0)
    return x


MU, SIGMA = np.array([40.0, -7.0, 3.1]), np.array([0.5, 2.0, 0.2])
WRAP3 = np.array([0, 0, 1], dtype=np.uint8)
EPS = 0.05


def gaussian_score(x):
    """The score of N(MU, diag SIGMA^2), the third column on the circle."""
    d = np.asarray(x, dtype=np.float64) - MU
    d[:, 2] = (d[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    return -d / SIGMA ** 2


def gaussian_case(n):
    """-> (start [n, 3] float32 with the third column in [-pi, pi), scale [3] = 1 / the start's spread)."""
    start = MU + np.array([3.0, 3.0, 0.6]) * SIGMA + 0.3 * SIGMA * np.random.RandomState(7).randn(n, 3)
    scale = 1.0 / start.std(0)
    start[:, 2] = (start[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    return start.astype(np.float32), scale


def gaussian_blocks(split):
    return [[0, 1], [2]] if split else [[0, 1, 2]]


def moments_against_the_target(x):
    """-> (|mean error| / sigma, std / sigma) per column, the third about MU on the circle."""
    d = np.asarray(x, dtype=np.float64) - MU
    d[:, 2] = (d[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    return np.abs(d.mean(0)) / SIGMA, d.std(0) / SIGMA


def assert_svgd_conditions(x, label):
    err, spread = moments_against_the_target(x)
    print("%s: |mean error| / sigma = %s, std / sigma = %s" % (label, np.round(err, 4), np.round(spread, 4)))
    assert np.all(err <= 0.1), (label, err)
    assert np.all((spread >= 0.6) & (spread <= 1.2)), (label, spread)


def assert_ascent_condition(x, label):
    d = np.asarray(x, dtype=np.float64) - MU
    d[:, 2] = (d[:, 2] + np.pi) % (2.0 * np.pi) - np.pi
    print("%s: max |x - mu| = %s" % (label, np.abs(d).max(0)))
    assert np.all(np.abs(d) <= EPS), (label, np.abs(d).max(0))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
NAMES = ("nfisam_sample_svgd", "nfisam_sample_svgd_scratch_count", "nfisam_sample_step")


def test_the_three_names_are_exported_and_declared():
    nh.build()
    lib = nh.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nfisam_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nfisam_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in nh.EXPORTS and name in declared and hasattr(lib, name), name
    assert lib.nfisam_abi_version() == 1600
    assert lib.nfisam_sample_svgd_scratch_count(130, 2, 5) == 3 * 5 * 3 * 64
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65535 * 64 + 1, 1, 1), (1, 65536, 1)):
        assert lib.nfisam_sample_svgd_scratch_count(*bad) == 0, bad


# ---- refusals before any launch ----------------------------------------------------------------------------------------------------
def test_check_svgd_blocks_refusals():
    t = nh.pack_mmd_blocks([2, 1], [1.0, 1.0])
    nh.check_svgd_blocks(t, [0, 1, 4], 5, scale=[1.0, 0.0, 2.0], wrap=[0, 0, 1])
    with pytest.raises(ValueError, match="1..65535 blocks"):
        nh.check_svgd_blocks(t[:0], [0, 1, 4], 5)
    bad = t.copy()
    bad["d"][1] = 0
    with pytest.raises(ValueError, match="leave the 3 entries"):
        nh.check_svgd_blocks(bad, [0, 1, 4], 5)
    for v in (0.0, -1.0, np.inf, np.nan):
        bad = t.copy()
        bad["inv_two_sigma2"][0] = v
        with pytest.raises(ValueError, match="positive and finite"):
            nh.check_svgd_blocks(bad, [0, 1, 4], 5)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_svgd_blocks(t, [0, 1, 5], 5)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_svgd_blocks(t, [-1, 1, 4], 5)
    with pytest.raises(ValueError, match="named more than once"):
        nh.check_svgd_blocks(t, [0, 1, 0], 5)
    with pytest.raises(ValueError, match="wrap must have one value per entry"):
        nh.check_svgd_blocks(t, [0, 1, 4], 5, wrap=[0, 1])
    with pytest.raises(ValueError, match="scale must have one value per entry"):
        nh.check_svgd_blocks(t, [0, 1, 4], 5, scale=[1.0, 1.0])
    with pytest.raises(ValueError, match="scale must be finite"):
        nh.check_svgd_blocks(t, [0, 1, 4], 5, scale=[1.0, np.nan, 1.0])
    bad = t.copy()
    bad["col_off"][1] = 1
    with pytest.raises(ValueError, match="share an entry"):
        nh.check_svgd_blocks(bad, [0, 1, 4], 5)
    with pytest.raises(ValueError, match="1-D numpy array"):
        nh.check_svgd_blocks(nh.pack_moment_blocks([2, 1]), [0, 1, 4], 5)


def test_bindings_refuse_bad_input_with_no_device():
    X, G = np.zeros((5, 3), dtype=np.float32), np.zeros((5, 3))
    t = nh.pack_mmd_blocks([3], [1.0])
    with pytest.raises(ValueError, match="shape of the points"):
        nh.svgd_direction(X, G[:, :2], t, [0, 1, 2], device="cuda")
    with pytest.raises(ValueError, match="no points"):
        nh.svgd_direction(X[:0], G[:0], t, [0, 1, 2], device="cuda")
    with pytest.raises(ValueError, match="named more than once"):
        nh.svgd_direction(X, G, t, [0, 1, 1], device="cuda")
    with pytest.raises(ValueError, match="tensors or arrays"):
        nh.svgd_direction(X[0], G[0], t, [0, 1, 2], device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.svgd_direction(X, G, t, [0, 1, 2], device="cpu")
    Xt, Gt = torch.zeros(3, 5), torch.zeros(3, 5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.svgd_direction_t(Xt, Gt, t, [0, 1, 2])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_step_t(Xt, [0, 1, 2], Gt, Gt.clone(), np.ones(3))
    for alpha in (-0.1, 1.0, np.nan):
        with pytest.raises(ValueError, match="alpha"):
            nh.check_step_args(alpha, 1e-6)
    for fudge in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="fudge"):
            nh.check_step_args(0.9, fudge)
    with pytest.raises(ValueError, match="eps must be finite"):
        nh.check_step_args(0.9, 1e-6, [1.0, np.inf])


def test_statistics_refuse_bad_options_with_no_device():
    x, s = np.zeros((6, 3), dtype=np.float32), np.zeros((6, 3))
    score = lambda p: np.zeros_like(p)
    with pytest.raises(ValueError, match="shape of x"):
        ST.stein_variational_direction(x, s[:, :2], [[0, 1, 2]])
    with pytest.raises(ValueError, match="points, columns"):
        ST.stein_variational_direction(x[0], s[0], [[0]])
    with pytest.raises(ValueError, match="overlapping blocks"):
        ST.stein_variational_direction(x, s, [[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="outside the 3 columns"):
        ST.stein_variational_direction(x, s, [[0, 3]])
    with pytest.raises(ValueError, match="non-empty list"):
        ST.stein_variational_direction(x, s, [[]])
    with pytest.raises(ValueError, match="no blocks"):
        ST.stein_variational_direction(x, s, [])
    for sigma in (0.0, -1.0, np.nan, [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="sigma is one positive bandwidth"):
            ST.stein_variational_direction(x, s, [[0, 1], [2]], sigma=sigma)
    with pytest.raises(ValueError, match="scale: one finite value per column"):
        ST.stein_variational_direction(x, s, [[0, 1, 2]], scale=[1.0, 1.0])
    with pytest.raises(ValueError, match="circular: one flag per column"):
        ST.stein_variational_direction(x, s, [[0, 1, 2]], circular=[True])
    ok = dict(blocks=[[0, 1, 2]], steps=3, step_size=0.1)
    for key, bad, match in (("steps", -1, "steps must be an integer >= 0"), ("steps", 1.5, "steps must be an integer >= 0"),
                            ("step_size", 0.0, "step_size"), ("step_size", np.inf, "step_size"),
                            ("step_size", [0.1, 0.1], "step_size"), ("sigma", -2.0, "sigma"), ("alpha", 1.0, "alpha"),
                            ("alpha", -0.5, "alpha"), ("fudge", 0.0, "fudge"), ("blocks", [[0, 1], [1]], "overlapping blocks")):
        with pytest.raises(ValueError, match=match):
            ST.stein_variational_refine(x, score, **dict(ok, **{key: bad}))
        with pytest.raises(ValueError, match=match):          # the options are refused before the CPU tensor is
            ST.stein_variational_refine_t(torch.zeros(3, 6), lambda Xt: None, **dict(ok, **{key: bad}))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.stein_variational_refine_t(torch.zeros(3, 6), lambda Xt: None, **ok)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.stein_variational_refine(x, score, device="cpu", **ok)
    with pytest.raises(ValueError, match="callable"):
        ST.stein_variational_refine(x, s, **ok)


def test_solver_methods_refuse_before_a_graph_exists():
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    solver = NFiSAM(NFiSAMArgs())
    with pytest.raises(RuntimeError, match="no factor graph yet"):
        solver.posterior_refine()
    with pytest.raises(RuntimeError, match="no factor graph yet"):
        solver.posterior_refine({}, steps=3, kernel="joint")
    with pytest.raises(RuntimeError, match="no factor graph yet"):
        solver.map_refine()
    with pytest.raises(RuntimeError, match="no factor graph yet"):
        solver.map_refine({}, top=2)


# ---- the restatement itself --------------------------------------------------------------------------------------------------------
def test_one_point_in_one_block_moves_along_its_score():
    rng = np.random.RandomState(3)
    x, g = rng.randn(1, 4).astype(np.float32) * 30, rng.randn(1, 4) * 10
    phi = direction(x, g, nh.pack_mmd_blocks([4], [0.7]), [2, 0, 3, 1], scale=[1.0, 0.0, 2.0, 0.5], wrap=[0, 1, 0, 0])
    assert np.array_equal(phi[:, 0], g[0, [2, 0, 3, 1]])                 # k_ii = 1, d_ii = 0


def test_wrapped_differences_push_apart_across_the_seam():
    x, g = np.array([[3.1], [-3.1]], dtype=np.float32), np.zeros((2, 1))
    t = nh.pack_mmd_blocks([1], [1.0])
    phi = direction(x, g, t, [0], wrap=[1])
    d = 2 * np.pi - (float(x[0, 0]) - float(x[1, 0]))                    # the short way round: 0.083 rad
    want = np.exp(-0.5 * d * d) * d / 2                                  # 2 inv = 1: point 1 (at -3.1) is pushed up, 0 down
    assert np.isclose(phi[0, 1], want, rtol=1e-12) and phi[0, 0] == -phi[0, 1]
    plain = direction(x, g, t, [0])
    # 6.2 rad apart without the wrap: exp(-6.2^2 / 2) 6.2 / 2 = 1.4e-8, out of the kernel's reach, and of the other sign
    assert 0 < plain[0, 0] < 1e-5 * abs(phi[0, 0]) and phi[0, 0] < 0


def test_step_rule_rounding_wrap_and_first():
    x = np.array([[100.0, 3.14], [-50.0, -3.14]], dtype=np.float32)
    phi, hist = np.array([[2.0, -1.0], [1.0, -4.0]]), np.array([[9.0, 9.0], [1.0, 1.0]])
    new, h = step(x, [0, 1], phi, hist, [0.5, 0.01], wrap=[0, 1], alpha=0.9, fudge=1e-6, first=False)
    assert np.allclose(h, 0.9 * hist + 0.1 * phi * phi, rtol=1e-15, atol=0.0)
    assert new.dtype == np.float32 and np.all(new[:, 1].astype(np.float64) >= -np.pi) and np.all(new[:, 1].astype(np.float64) < np.pi)
    assert new[0, 1] < 0 and new[1, 1] > 0                               # both stepped across the seam
    first, h1 = step(x, [0, 1], phi, hist * np.nan, [0.5, 0.01], wrap=[0, 1], first=True)
    assert np.array_equal(h1, phi * phi) and np.all(np.isfinite(first))
    # a value that rounds to +-float32(pi) is brought to the float32 just inside -pi
    edge, _ = step(np.array([[np.float32(np.pi)]]), [0], np.array([[1.0]]), None, [1e-12], wrap=[1], first=True)
    assert edge[0, 0] == INSIDE and float(INSIDE) > -np.pi
    # a step below the float32 spacing is lost: 7.6e-6 at 100 m
    lost, _ = step(np.array([[100.0]], dtype=np.float32), [0], np.array([[1.0]]), None, [3e-6], first=True)
    assert lost[0, 0] == np.float32(100.0) and np.spacing(np.float32(100.0)) == np.float32(7.6293945e-06)


@pytest.mark.parametrize("n", (65, 130))
@pytest.mark.parametrize("split", (False, True))
def test_restatement_meets_the_svgd_conditions(n, split):
    start, scale = gaussian_case(n)
    blocks = gaussian_blocks(split)
    flat = np.concatenate(blocks)
    table = nh.pack_mmd_blocks([len(b) for b in blocks], [np.sqrt(len(b)) for b in blocks])
    x = refine(start, gaussian_score, table, flat, np.full(3, EPS), 500, scale=scale[flat], wrap=WRAP3[flat])
    assert_svgd_conditions(x, "numpy, n = %d, %s" % (n, "blocks {0, 1}, {2}" if split else "one joint block"))


def test_restatement_meets_the_ascent_condition():
    start, scale = gaussian_case(65)
    x = refine(start, gaussian_score, nh.pack_mmd_blocks([3], [1.0]), [0, 1, 2], np.full(3, EPS), 300, wrap=WRAP3, kernel=False)
    assert_ascent_condition(x, "numpy ascent")
