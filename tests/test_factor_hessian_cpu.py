"""The curvature row of value / score / curvature, without a device: `Factors.*.hess_x_log_pdf` against the 60-digit Hessians of
tests/golden/factor_hessian_exact.npz (tests/golden/make_factor_hessian_fixture.py: mpmath, the cases and points of
factor_exact.npz), the small-angle series of a'' and l'', and the matrix-free solvers of utils/Statistics.py on CPU tensors.

The bound is that of tests/test_factor_exact_cpu.py, |got - exact| <= C x 2^-53 x scale with the same C = 256 and no allowance:
a Hessian is the derivative of the score's smooth formula.  Largest ratios measured here (numpy float64) are printed per case
and recorded next to the device's in profiles/factor_hessian.json: 6.5 over the cases (se2_prior_medium), 2.8 on the joint
H v of the whole graphs (Manhattan-136); a'' and l'' alone 22 and 52, on the plain side of the switch |w| = 0.6 (the header's
balance expects up to 33 and 67 there)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from factors import Factors as F
from test_factor_density_cpu import factor_columns
from test_factor_exact_cpu import C, CAP, EPS, EXACT, GOLDEN, W_LIST, exact_cases, exact_fixture, exact_graph, ratio
from utils import Statistics as ST

HESSIAN = os.path.join(GOLDEN, "factor_hessian_exact.npz")


# ---- shared with tests/test_factor_hessian_gpu.py -------------------------------------------------------------------------------
def hessian_fixture():
    return np.load(HESSIAN)


def hessian_cases(hx=None, names=None):
    """The cases of factor_exact.npz with .hess / .hess_scale [m, w, w] from the Hessian fixture."""
    hx = hessian_fixture() if hx is None else hx
    cases = exact_cases(names=names)
    for c in cases:
        c.hess, c.hess_scale = hx[c.name + "_hess"], hx[c.name + "_hess_scale"]
        assert c.hess.shape == c.hess_scale.shape == (c.x.shape[0], c.x.shape[1], c.x.shape[1])
    return cases


def host_hessian(c):
    x = c.x.astype(np.float64)
    if len(c.factors) == 1:
        return c.factors[0].hess_x_log_pdf(x)
    return np.concatenate([f.hess_x_log_pdf(x[i:i + 1]) for i, f in enumerate(c.factors)])


def hessian_graph(hx, key):
    """(factors, col, x float32 [n, total], v [total], hv, hv_scale [n, total]) of a whole graph of the Hessian fixture."""
    fx = exact_fixture()
    factors, col, x, _ = exact_graph(fx, key)
    rows = hx[key + "_rows"]
    pick = [int(np.flatnonzero(fx[key + "_rows"] == r)[0]) for r in rows]
    return factors, col, x[pick], hx[key + "_v"], hx[key + "_hv"], hx[key + "_hv_scale"].astype(np.float64)


def load_generator():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_factor_hessian_fixture", os.path.join(GOLDEN, "make_factor_hessian_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the fixture keeps the conditions its generator asserts -----------------------------------------------------------------------
def test_fixture_meets_its_own_caps():
    hx, fx = hessian_fixture(), exact_fixture()
    cases = hessian_cases(hx)
    exempt = set(str(s) for s in hx["exempt"])
    assert [c.name for c in cases] == [str(n) for n in fx["cases"]] and exempt < set(c.name for c in cases)
    assert len(hx["exempt_reason"]) == len(exempt) and all(len(str(r)) > 10 for r in hx["exempt_reason"])
    assert exempt - set(str(s) for s in fx["exempt"]) == {"a004"}                    # one further case, justified there
    assert os.path.getsize(HESSIAN) <= os.path.getsize(EXACT)
    for c in cases:
        assert (~c.mask).sum() <= 0.05 * c.mask.size, c.name                         # the masked rows: unchanged
        assert not c.hess[~c.mask].any() and not c.hess_scale[~c.mask].any(), c.name
        h, s = c.hess[c.mask], c.hess_scale[c.mask]
        assert np.all(np.isfinite(h)) and np.all(np.isfinite(s)) and np.all(s >= 0)
        assert np.array_equal(s, s.transpose(0, 2, 1)), c.name                       # one bound for [r, c] and [c, r]
        assert ratio(h.transpose(0, 2, 1), h, s) <= 1e-3, c.name                     # symmetric far below a rounding
        if c.name not in exempt:
            assert np.mean(C * EPS * s <= CAP * (np.abs(h) + 1.0)) >= 0.9, c.name
    for key, width in (("ksd", 13), ("manhattan136", None)):
        v, hv, sc = hx[key + "_v"], hx[key + "_hv"], hx[key + "_hv_scale"]
        assert hv.shape == sc.shape == (len(hx[key + "_rows"]), v.size) and (width is None or v.size == width)
        assert np.all(np.isfinite(hv)) and np.mean(C * EPS * sc <= CAP * (np.abs(hv) + 1.0)) >= 0.9
        assert set(hx[key + "_rows"]) <= set(fx[key + "_rows"])
    assert len(hx["ksd_rows"]) == 64 and np.array_equal(hx["manhattan136_rows"], fx["manhattan136_rows"][::6])


def test_generator_reproduces_a_dozen_stored_values():
    gen = load_generator()
    cases = {c.name: c for c in hessian_cases()}
    made = {name: (cls, params, x) for name, cls, params, x in gen.base.all_cases()}
    picks = [("a000", 3), ("a005", 17), ("a018", 9), ("a024", 23), ("se2_prior_tight", 2), ("se2_rel_medium", 11), ("se2_rel_full", 40),
             ("range_pose_edges", 2), ("ring_far_centre", 0), ("mix_k3_ahead", 4), ("mix_twice", 7), ("r2_prior_corr", 5)]
    for name, i in picks:
        cls, params, x = made[name]
        c = cases[name]
        assert np.array_equal(x, c.x)
        got = gen.hessian(cls, params[i % params.shape[0]], x[i])
        assert bool(got["mask"]) == bool(c.mask[i])
        assert np.array_equal(np.array([[float(t) for t in row] for row in got["hess"]]), c.hess[i]), (name, i)
        assert np.array_equal(np.array([gen.base.up64(row) for row in got["hess_scale"]]), c.hess_scale[i]), (name, i)
        gen.cross_check(cls, params[i % params.shape[0]], x[i], got, (name, i))       # and mpmath.diff of the definition agrees


# ---- Factors.hess_x_log_pdf against the 60-digit values ------------------------------------------------------------------------------
def test_every_host_hessian_is_within_c_roundings_and_symmetric():
    worst, seen = {}, set()
    for c in hessian_cases():
        H = host_hessian(c)
        assert H.dtype == np.float64 and H.shape == c.hess.shape and np.all(np.isfinite(H))
        m = c.mask
        worst[c.name] = ratio(H[m], c.hess[m], c.hess_scale[m])
        assert ratio(H[m].transpose(0, 2, 1), H[m], 2.0 * c.hess_scale[m]) <= C, c.name       # symmetric within the same bound
        if not isinstance(c.factors[0], F.BinaryFactorMixture):
            assert not H[~m].any(), c.name                                            # a range of exactly 0: the zero block
        seen.add(c.cls)
        print("%-26s %-42s |got - exact| / (2^-53 scale): %8.3g" % (c.name, c.cls, worst[c.name]))
    print("largest ratio: %.3g (C = %g)" % (max(worst.values()), C))
    assert len(seen) == 9
    bad = {k: v for k, v in worst.items() if v > C}
    assert not bad, bad


@pytest.mark.parametrize("key", ["ksd", "manhattan136"])
def test_whole_graph_joint_product(key):
    factors, col, x, v, hv, scale = hessian_graph(hessian_fixture(), key)
    x64 = x.astype(np.float64)
    got = np.zeros_like(hv)
    for f in factors:                                                                # table order: the order of the fixture's sums
        cols = factor_columns(f, col)
        got[:, cols] = got[:, cols] + f.hess_x_log_pdf(x64[:, cols]) @ v[cols]
    r = ratio(got, hv, scale)
    print("%s: %d factors x %d points: |H v - exact| / (2^-53 scale): %.3g" % (key, len(factors), x.shape[0], r))
    assert r <= C


# ---- the small-angle terms on their own ------------------------------------------------------------------------------------------------
def test_log_map_curvature_matches_mpmath_at_every_branch_edge_and_across_the_switch():
    """a'' = (a - 1) / (2 sin^2 h) and l'' = (1 / sin^2 h - 1 / h^2) / 2 of `Factors._log_map_curvature` (the numpy restatement
    of csrc/factor_model.h: log_map_curvature) at the w list of the fixture and on both sides of the series switch |h| = 0.3,
    both signs, against mpmath at 60 digits.  w is the input here, so a term's scale is its own magnitude; the same C."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    edge = 2.0 * F._SERIES2_H
    w = np.array([s * t for t in W_LIST + [float(np.nextafter(edge, 0.0)), edge, 0.5, 0.59, 0.61, 0.7] for s in (1.0, -1.0)])
    assert np.sum(np.abs(0.5 * w) < F._SERIES2_H) >= 20 and np.sum(np.abs(0.5 * w) >= F._SERIES2_H) >= 10
    a = F._log_map_terms(w)[0]
    dda, ddl = F._log_map_curvature(w, a)
    worst = np.zeros(2)
    with mp.workdps(60):
        for i, wi in enumerate(w):
            if wi == 0.0:
                assert dda[i] == -1.0 / 6.0 and ddl[i] == 1.0 / 6.0
                continue
            h = mpmath.mpf(float(wi)) / 2
            s2 = 1 / mpmath.sin(h) ** 2
            exact = ((h * mpmath.cot(h) - 1) * s2 / 2, (s2 - 1 / h ** 2) / 2)
            for j, (got, ex) in enumerate(zip((dda[i], ddl[i]), exact)):
                worst[j] = max(worst[j], float(abs(mpmath.mpf(float(got)) - ex) / (abs(ex) * EPS)))
    print("|got - exact| / (2^-53 |exact|): a'' %.3g, l'' %.3g" % tuple(worst))
    assert worst.max() <= C, worst


# ---- the matrix-free solvers on CPU tensors -------------------------------------------------------------------------------------------
def test_check_newton_options_refusals():
    ok = ST.check_newton_options(5, steps=3, damping=0.5, circular=[0, 0, 1, 0, 0])
    assert ok["cg_iters"] == 5 and ok["damping"].shape == (5,) and ok["flags"][2] and ok["gtol"] == ST.NEWTON_GTOL
    assert ok["backtracks"] == ST.NEWTON_BACKTRACKS == 10 and np.array_equal(ok["scale"], np.ones(5))
    for bad in (dict(steps=-1), dict(steps=1.5), dict(steps=True), dict(cg_iters=0), dict(rtol=0.0), dict(rtol=1.0),
                dict(rtol=np.nan), dict(damping=-1.0), dict(damping=np.inf), dict(damping=[0.0, 1.0]), dict(gtol=0.0),
                dict(gtol=np.inf), dict(backtracks=-1), dict(backtracks=61), dict(scale=[1.0] * 4), dict(scale=[-1.0] * 5),
                dict(circular=[1, 0])):
        with pytest.raises(ValueError):
            ST.check_newton_options(5, **bad)
    with pytest.raises(ValueError):
        ST.check_newton_options(0)
    with pytest.raises(ValueError):
        ST.conjugate_gradient_t(lambda V: V, torch.zeros(3, 2), 3, 1e-8)              # float32
    with pytest.raises(ValueError):
        ST.newton_refine_t(torch.zeros(3, 2, dtype=torch.float64), lambda X, V: (V, V), lambda X: X[0], 1)
    with pytest.raises(ValueError):
        ST.newton_refine_t(torch.zeros(3, 2), None, lambda X: X[0], 1)


def _spd(rng, D, lo=0.5, hi=20.0):
    q, _ = np.linalg.qr(rng.randn(D, D))
    return (q * np.exp(rng.uniform(np.log(lo), np.log(hi), D))) @ q.T


def test_conjugate_gradient_meets_rtol_within_d_iterations_and_freezes_stopped_points():
    rng = np.random.RandomState(11)
    D, n = 9, 7
    A = _spd(rng, D)
    At = torch.from_numpy(A)
    B = torch.from_numpy(rng.randn(D, n))
    B[:, 3] = 0.0                                                                    # b = 0: solved before the first product
    calls = []

    def hvp(V):                                                                      # H = -A: a log density's Hessian at a mode
        calls.append(1)
        return -(At @ V)
    out = ST.conjugate_gradient_t(hvp, B, D, 1e-10)
    assert len(calls) <= D and out["x"].dtype == torch.float64
    assert float(out["residual"].max()) <= 1e-10 and not out["negative_curvature"].any()
    assert int(out["iters"][3]) == 0 and not out["x"][:, 3].any() and int(out["iters"].max()) <= D
    exact = np.linalg.solve(A, B.numpy())
    assert np.abs(out["x"].numpy() - exact).max() <= np.linalg.cond(A) * 1e-10 * np.abs(exact).max()
    # an easy point (b an eigenvector: one iteration) stops at once and leaves the others' bits alone
    w, q = np.linalg.eigh(A)
    B2 = B.clone()
    B2[:, 0] = torch.from_numpy(q[:, 2])
    out2 = ST.conjugate_gradient_t(hvp, B2, D, 1e-10)
    assert int(out2["iters"][0]) == 1 and np.allclose(out2["x"][:, 0].numpy(), q[:, 2] / w[2], rtol=1e-12, atol=0.0)
    assert torch.equal(out2["x"][:, 1:], out["x"][:, 1:]) and torch.equal(out2["residual"][1:], out["residual"][1:])
    # damping: (A + diag(d)) x = b
    d = rng.uniform(0.0, 3.0, D)
    out3 = ST.conjugate_gradient_t(hvp, B, D, 1e-10, damping=d)
    assert np.abs(out3["x"].numpy() - np.linalg.solve(A + np.diag(d), B.numpy())).max() <= 1e-8
    # a budget too small: the point reports the residual it has
    short = ST.conjugate_gradient_t(hvp, B, 2, 1e-10)
    assert int(short["iters"].max()) == 2 and float(short["residual"][0]) > 1e-10


def test_conjugate_gradient_flags_negative_curvature():
    rng = np.random.RandomState(12)
    D = 6
    A = _spd(rng, D)
    w, q = np.linalg.eigh(A)
    M = A - (w[0] + 5.0) * np.outer(q[:, 0], q[:, 0])                                # one eigenvalue of -5: indefinite
    Mt = torch.from_numpy(M)
    B = torch.from_numpy(np.stack([q[:, 0], q[:, 3], q[:, 0] + q[:, 1]], 1))          # along it, away from it, across
    out = ST.conjugate_gradient_t(lambda V: -(Mt @ V), B, D, 1e-10)
    neg = out["negative_curvature"].numpy()
    assert neg[0] and not neg[1] and neg[2]
    assert torch.equal(out["x"][:, 0], B[:, 0]) and int(out["iters"][0]) == 0          # first iteration: b itself
    assert np.allclose(out["x"][:, 1].numpy(), q[:, 3] / w[3], rtol=1e-12, atol=1e-15)
    assert np.all(np.isfinite(out["x"].numpy()))


def test_newton_refine_on_a_quadratic_and_on_an_indefinite_one():
    rng = np.random.RandomState(13)
    D, n = 5, 6
    A = _spd(rng, D, 0.5, 8.0)
    At, m = torch.from_numpy(A), torch.from_numpy(rng.randn(D, 1) * 3.0)
    X0 = torch.from_numpy((rng.randn(D, n) * 5.0).astype(np.float32))

    def score_hvp(Xt, Vt):
        return -(At @ Vt), -(At @ (Xt.double() - m))

    def log_p(Xt):
        d = Xt.double() - m
        return -0.5 * (d * (At @ d)).sum(0)
    # the floor: the score at the float32 point next to the mode is at most |A| times half the spacing of the coordinate
    floor = float(np.abs(A).sum(1).max() * 2.0 ** -24 * max(float(m.abs().max()), 1.0))
    X = X0.clone()
    out = ST.newton_refine_t(X, score_hvp, log_p, 4, rtol=1e-12, gtol=2.0 * floor)
    assert out["steps"] == 1 and bool(out["converged"].all()) and not out["negative_curvature"].any()
    assert np.abs(X.numpy() - m.numpy()).max() <= 2.0 ** -23 * max(float(m.abs().max()), 1.0)
    assert torch.equal(out["log_p"], log_p(X)) and bool((out["log_p"] >= out["start_log_p"]).all())
    still = X0.clone()
    zero = ST.newton_refine_t(still, score_hvp, log_p, 0)
    assert zero["steps"] == 0 and torch.equal(still, X0) and torch.equal(zero["log_p"], zero["start_log_p"])
    # a heading is wrapped into [-pi, pi) as it is stored: log p = cos(x0 - 4) - (x1 - 1)^2 / 2, one step from (3, 0)
    Y = torch.tensor([[3.0], [0.0]], dtype=torch.float32)

    def periodic(Xt, Vt):
        x = Xt.double()
        return (torch.stack([-torch.cos(x[0] - 4.0) * Vt[0], -Vt[1]]), torch.stack([-torch.sin(x[0] - 4.0), -(x[1] - 1.0)]))
    ST.newton_refine_t(Y, periodic, lambda Xt: torch.cos(Xt.double()[0] - 4.0) - 0.5 * (Xt.double()[1] - 1.0) ** 2, 1,
                       circular=[1, 0], backtracks=0)
    step = 3.0 + np.sin(1.0) / np.cos(1.0)                                          # 4.557: stored as 4.557 - 2 pi
    assert float(Y[0, 0]) == float(np.float32(step - 2.0 * np.pi)) and float(Y[1, 0]) == 1.0
    # an indefinite Hessian: flagged, and no point falls
    w, q = np.linalg.eigh(A)
    Mt = torch.from_numpy(A - (w[0] + 3.0) * np.outer(q[:, 0], q[:, 0]))
    X = X0.clone()
    out = ST.newton_refine_t(X, lambda Xt, Vt: (-(Mt @ Vt), -(Mt @ (Xt.double() - m))),
                             lambda Xt: -0.5 * ((Xt.double() - m) * (Mt @ (Xt.double() - m))).sum(0), 2, gtol=2.0 * floor)
    assert bool(out["negative_curvature"].any()) and bool((out["log_p"] >= out["start_log_p"]).all())


def test_coloured_probes_read_the_diagonal_and_precondition_an_ill_scaled_chain():
    """A chain whose variables are known to millimetres at one end and to metres at the other, as a SLAM graph's are: plain
    conjugate gradients do not arrive within D products, the iteration preconditioned with the probed diagonal does better by
    orders of magnitude; the classes of `probe_colours` show diag(H) exactly (0/1 probes pick single entries)."""
    rng = np.random.RandomState(14)
    D = 24
    sig = np.exp(rng.uniform(np.log(4e-3), np.log(2.0), D))
    L = np.eye(D)
    for i in range(D - 1):
        L[i + 1, i] = -0.9
    A = (L / sig[:, None]).T @ (L / sig[:, None])
    At = torch.from_numpy(A)
    hvp = lambda V: -(At @ V)
    colours = ST.probe_colours([[i, i + 1] for i in range(D - 1)], D)
    assert len(colours) == 2 and np.array_equal(np.sort(np.concatenate(colours)), np.arange(D))
    for g in ([0, 1, 2], [2, 5]):                                                    # no class holds two coupled columns
        assert all(len(set(g) & set(c.tolist())) <= 1 for c in ST.probe_colours([[0, 1, 2], [2, 5]], 6))
    with pytest.raises(ValueError):
        ST.probe_colours([[0, 6]], 6)
    diag = ST.hessian_diagonal_t(hvp, colours, D, 3, "cpu")
    assert np.array_equal(diag.numpy(), -np.diag(A)[:, None] * np.ones((1, 3)))
    B = torch.eye(D, dtype=torch.float64)
    inv = np.linalg.inv(A)
    plain = ST.conjugate_gradient_t(hvp, B, D, 1e-8)
    minv = ST.inverse_diagonal(ST.hessian_diagonal_t(hvp, colours, D, D, "cpu"), None)
    pre = ST.conjugate_gradient_t(hvp, B, D, 1e-8, precond=minv)
    err = lambda r: float(np.abs(r["x"].numpy() - inv).max() / np.abs(inv).max())
    print("D = %d, cond %.3g: after D products plain CG residual %.3g error %.3g, preconditioned residual %.3g error %.3g"
          % (D, np.linalg.cond(A), float(plain["residual"].max()), err(plain), float(pre["residual"].max()), err(pre)))
    assert err(pre) < err(plain) and float(plain["residual"].max()) > 1e-8          # the claim above, no more
    # in exact arithmetic D products end either iteration; in float64 the preconditioned one is given 4 D and must arrive
    more = ST.conjugate_gradient_t(hvp, B, 4 * D, 1e-8, precond=minv[:, :1].contiguous())      # [D, 1]: one diagonal for all
    assert float(more["residual"].max()) <= 1e-8 and not more["negative_curvature"].any()
    assert err(more) <= np.linalg.cond(A) * 1e-8
    assert torch.equal(ST.inverse_diagonal(torch.tensor([[-4.0, 2.0, 0.0]], dtype=torch.float64).t(), None),
                       torch.tensor([[0.25, 1.0, 1.0]], dtype=torch.float64).t())   # no curvature of the right sign: unscaled
    with pytest.raises(ValueError):
        ST.conjugate_gradient_t(hvp, B, D, 1e-8, precond=minv[:3])
