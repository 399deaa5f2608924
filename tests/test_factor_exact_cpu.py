"""The host factor formulas against 60-digit values: `Factors.*.log_pdf` and `grad_x_log_pdf` of every class against
tests/golden/factor_exact.npz, which tests/golden/make_factor_exact_fixture.py computes from the mathematics alone (mpmath,
60 digits, the smooth density without small-angle branches, built from the constructor parameters: the packing is graded too).

The bound, for every value:   |got - exact| <= C x 2^-53 x scale + allow
  * `scale` is the fixture's running error bound of that value: the same expression with every difference replaced by the sum
    of the absolute values, carried from the inputs on (the generator's docstring has the rules);
  * `allow` is the documented flat spot of the VALUE's own branch, w^2 / 12 where |w| < 1e-5, and 0 everywhere else; a score has
    none (csrc/factor_score.hip promises the smooth derivative everywhere);
  * C = 256 is derived, not fitted: csrc/factor_model.h documents a worst loss of 1.5 eps / h^2 = 150 eps in a, a' and l' at
    the series switch |h| = 0.1; the remaining operations and library functions along the longest chain (two wraps of a
    heading, sin / cos, two rotations, nine products of the quadratic form, the log, exp and division of a mixture), a few
    roundings each, come to about a hundred; rounded up to the next power of two.
A ratio |got - exact| / (2^-53 scale) above 256 is a finding: the generator's scale misses a term, or a formula loses digits.
Largest ratios measured here (the host, numpy float64) are printed per case by the tests and recorded next to the device's
in profiles/factor_exact.json: 3.8 on a value (a range factor with a measured range of 0) and 3.5 on a score (the mixture with
a candidate listed twice) over the cases, 5.8 over the whole graphs (a term of Manhattan-136); da / dw of `_log_map_terms` alone
188 at w = 0.2, the first argument of the plain form.  Before the |w| < 1e-10 branch of the value kept its off-diagonal term
(csrc/factor_model.h) the SE(2) sweeps stood at up to 7.2e4."""
import importlib.util
import os

import numpy as np
import pytest

from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from test_factor_density_cpu import GRAPHS, build_case, factor_columns, fixture, load_graph
from test_factor_score_cpu import host_joint_score, ksd_graph, score_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXACT = os.path.join(GOLDEN, "factor_exact.npz")
C = 256.0
EPS = 2.0 ** -53
CAP, VACUOUS = 1e-9, 0.25
W_LIST = [0.0, 1e-12, 9.9e-11, 1.01e-10, 1e-8, 9.9e-6, 1.01e-5, 1e-4, 1e-3, 0.05, float(np.nextafter(0.2, 0.0)), 0.2, 0.21, 1.0,
          3.0, float(np.pi) - 1e-3, float(np.pi) - 1e-5]
SE2_CLASSES = ("UnarySE2ApproximateGaussianPriorFactor", "SE2RelativeGaussianLikelihoodFactor")


# ---- shared with tests/test_factor_exact_gpu.py ---------------------------------------------------------------------------------
def exact_fixture():
    return np.load(EXACT)


def exact_factor(cls, params):
    """The factor of a case from its constructor parameters (the generator's layouts)."""
    if cls == "AmbiguousDataAssociationFactor" and len(params) > 3 + int(params[0]):
        k = int(params[0])
        idx = [int(v) for v in params[3 + k:3 + 2 * k]]
        L = [R2Variable("L%d" % i, VariableType.Landmark) for i in range(max(idx) + 1)]
        return F.AmbiguousDataAssociationFactor(SE2Variable("X0"), [L[i] for i in idx], np.array(params[1:1 + k]),
                                                F.SE2R2RangeGaussianLikelihoodFactor, float(params[1 + k]), float(params[2 + k]))
    return build_case(cls, params)


class ExactCase(object):
    """A case of the fixture: `factors[i % len(factors)]` belongs to row i of x."""

    def __init__(self, fx, dens, name):
        self.name = name
        if name + "_cls" in fx.files:
            self.cls, params, self.x = str(fx[name + "_cls"]), fx[name + "_params"], fx[name + "_x"]
        else:                                                        # a part-(a) case of factor_density.npz, read from there
            i = int(name[1:])
            self.cls, params, self.x = str(dens["a_classes"][i]), dens["a%03d_params" % i][None, :], dens["a%03d_x" % i]
        self.factors = [exact_factor(self.cls, p) for p in params]
        for key in ("logp", "logp_scale", "logp_allow", "score", "score_scale", "mask"):
            setattr(self, key, fx[name + "_" + key])
        self.score_scale = self.score_scale.astype(np.float64)
        self.w = fx[name + "_w"] if name + "_w" in fx.files else None
        assert self.x.dtype == np.float32 and self.score.shape == self.x.shape and len(self.factors) in (1, self.x.shape[0])

    def host(self):
        """(log_pdf [n], grad_x_log_pdf [n, width]) of the host formulas at the case's points."""
        x = self.x.astype(np.float64)
        if len(self.factors) == 1:
            return self.factors[0].log_pdf(x), self.factors[0].grad_x_log_pdf(x)
        return (np.concatenate([f.log_pdf(x[i:i + 1]) for i, f in enumerate(self.factors)]),
                np.concatenate([f.grad_x_log_pdf(x[i:i + 1]) for i, f in enumerate(self.factors)]))


def exact_cases(fx=None, names=None):
    fx = exact_fixture() if fx is None else fx
    dens = fixture()
    return [ExactCase(fx, dens, str(n)) for n in fx["cases"] if names is None or str(n) in names]


def ratio(got, exact, scale, allow=0.0):
    """largest (|got - exact| - allow) / (2^-53 scale); where the scale is 0 (a masked score, a column the factor does not
    depend on) only the exact value itself passes."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), exact.shape)
    assert got.shape == exact.shape and np.all(np.isfinite(exact)) and np.all(scale >= 0)
    if not exact.size:
        return 0.0
    err = np.maximum(np.abs(got - exact) - allow, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / (EPS * scale), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


def exact_graph(fx, key):
    """(factors, col, x float32 [n, total], and the fixture's arrays of the graph as a dict)."""
    if key == "ksd":
        fs = score_fixture()
        variables, factors = ksd_graph(fs["ksd_truth"])
        col, off = {}, 0
        for v in variables:
            col[v] = off
            off += v.dim
        x = fs["ksd_samples"][fx["ksd_rows"]]
    else:
        nodes, factors, col, x, _, _ = load_graph(fixture(), key)
        x = x[fx[key + "_rows"]]
    keys = ("terms", "terms_scale", "terms_allow", "total", "total_scale", "total_allow", "score", "score_scale")
    return factors, col, x, {k: fx[key + "_" + k].astype(np.float64) for k in keys}


def load_generator():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_factor_exact_fixture", os.path.join(GOLDEN, "make_factor_exact_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the fixture keeps the conditions its generator asserts -----------------------------------------------------------------------
def test_fixture_meets_its_own_conditions():
    fx = exact_fixture()
    cases = exact_cases(fx)
    exempt = set(str(s) for s in fx["exempt"])
    assert len(cases) == len(fx["cases"]) >= 28 + 6 and exempt < set(c.name for c in cases) and len(fx["exempt_reason"]) == len(exempt)
    assert [c.name for c in cases[:28]] == ["a%03d" % i for i in range(28)]           # every part-(a) case, unchanged
    assert os.path.getsize(EXACT) < os.path.getsize(os.path.join(GOLDEN, "factor_score.npz"))
    seen = set()
    for c in cases:
        seen.add(c.cls)
        assert c.x.shape[0] <= 64, c.name
        assert (~c.mask).sum() <= 0.05 * c.mask.size, c.name
        assert np.all(c.score[~c.mask] == 0.0) and np.all(c.score_scale[~c.mask] == 0.0)
        if c.w is not None:
            assert np.all(np.pi - np.abs(c.w) > 1e-6), c.name                          # nothing on the heading wrap
            assert np.allclose(c.logp_allow, np.where(np.abs(c.w) < 1e-5, c.w * c.w / 12.0, 0.0), rtol=1e-14, atol=0.0)
        else:
            assert not c.logp_allow.any()
        for exact, scale in ((c.logp, c.logp_scale), (c.score[c.mask], c.score_scale[c.mask])):
            bound = C * EPS * scale
            assert np.all(np.isfinite(exact)) and np.all(bound <= VACUOUS * (np.abs(exact) + 1.0)), c.name    # never vacuous
            if c.name not in exempt:
                assert np.mean(bound <= CAP * (np.abs(exact) + 1.0)) >= 0.9, c.name
    assert len(seen) == 9                                                              # every class
    targets = np.array([s * w for w in W_LIST for s in (1.0, -1.0)])
    for name in ("se2_prior_tight", "se2_prior_medium", "se2_prior_full", "se2_rel_tight", "se2_rel_medium", "se2_rel_full"):
        w = next(c for c in cases if c.name == name).w
        near = np.abs(w[None, :] - targets[:, None]).min(1)
        assert np.all(near <= 1e-15 + 1e-15 * np.abs(targets) * 16), name                 # w landed on every target


# ---- Factors.log_pdf / grad_x_log_pdf against the 60-digit values ------------------------------------------------------------------
def test_every_case_is_within_c_roundings_of_the_exact_value():
    worst = {}
    for c in exact_cases():
        logp, grad = c.host()
        assert logp.dtype == grad.dtype == np.float64
        r_v, r_g = ratio(logp, c.logp, c.logp_scale, c.logp_allow), ratio(grad[c.mask], c.score[c.mask], c.score_scale[c.mask])
        assert np.all(np.isfinite(grad))
        if c.cls not in ("AmbiguousDataAssociationFactor", "BinaryFactorWithNullHypo"):
            assert np.all(grad[~c.mask] == 0.0), c.name                               # a range of exactly 0: the zero vector
        worst[c.name] = (r_v, r_g)
        print("%-26s %-42s |got - exact| / (2^-53 scale): value %8.3g  score %8.3g" % (c.name, c.cls, r_v, r_g))
    print("largest ratio: value %.3g, score %.3g (C = %g)" % (max(v for v, g in worst.values()), max(g for v, g in worst.values()), C))
    bad = {k: v for k, v in worst.items() if max(v) > C}
    assert not bad, bad


@pytest.mark.parametrize("key", sorted(GRAPHS) + ["ksd"])
def test_whole_graph_terms_totals_and_joint_score(key):
    fx = exact_fixture()
    factors, col, x, ex = exact_graph(fx, key)
    x64 = x.astype(np.float64)
    terms = np.stack([f.log_pdf(x64[:, factor_columns(f, col)]) for f in factors])
    tot = np.zeros(x.shape[0])
    for t in terms:
        tot = tot + t
    r = (ratio(terms, ex["terms"], ex["terms_scale"], ex["terms_allow"]), ratio(tot, ex["total"], ex["total_scale"], ex["total_allow"]),
         ratio(host_joint_score(factors, col, x), ex["score"], ex["score_scale"]))
    print("%s: %d factors x %d points: |got - exact| / (2^-53 scale): terms %.3g, totals %.3g, joint score %.3g"
          % (key, len(factors), x.shape[0], *r))
    assert max(r) <= C, r


def test_value_and_score_see_the_same_residual():
    """At |w| >= 1e-3 the value has no allowance: the value the host matches and the score the host matches are the density and
    the gradient of one function of one residual."""
    rows = 0
    for c in exact_cases():
        if c.w is None:
            continue
        big = np.abs(c.w) >= 1e-3
        assert not c.logp_allow[big].any()
        logp, grad = c.host()
        assert ratio(logp[big], c.logp[big], c.logp_scale[big]) <= C and ratio(grad[big], c.score[big], c.score_scale[big]) <= C
        rows += int(big.sum())
    assert rows >= 200


# ---- the small-angle terms on their own ------------------------------------------------------------------------------------------------
def test_log_map_terms_match_mpmath_at_every_branch_edge():
    """a = h cot h, da / dw and d logdet / dw of `Factors._log_map_terms` at the w list of the fixture, both signs, against
    mpmath at 60 digits.  w is the input here, so a term's scale is its own magnitude; the same C."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    w = np.array([s * v for v in W_LIST for s in (1.0, -1.0)])
    a, da, dl = F._log_map_terms(w)
    worst = np.zeros(3)
    with mp.workdps(60):
        for i, wi in enumerate(w):
            if wi == 0.0:
                assert a[i] == 1.0 and da[i] == 0.0 and dl[i] == 0.0
                continue
            h = mpmath.mpf(float(wi)) / 2
            cot = mpmath.cot(h)
            exact = (h * cot, (cot - h / mpmath.sin(h) ** 2) / 2, 1 / h - cot)
            for j, (got, ex) in enumerate(zip((a[i], da[i], dl[i]), exact)):
                worst[j] = max(worst[j], float(abs(mpmath.mpf(float(got)) - ex) / (abs(ex) * EPS)))
    print("|got - exact| / (2^-53 |exact|): a %.3g, da/dw %.3g, dlogdet/dw %.3g" % tuple(worst))
    assert worst.max() <= C, worst


# ---- the committed file is what the generator writes --------------------------------------------------------------------------------------
def test_generator_reproduces_a_dozen_stored_values():
    gen = load_generator()
    fx = exact_fixture()
    cases = {c.name: c for c in exact_cases(fx)}
    made = {name: (cls, params, x) for name, cls, params, x in gen.all_cases()}
    assert list(made) == [str(n) for n in fx["cases"]]
    picks = [("a000", 3), ("a005", 17), ("a018", 9), ("a024", 23), ("se2_prior_tight", 2), ("se2_rel_medium", 11), ("se2_rel_full", 40),
             ("range_pose_edges", 2), ("ring_far_centre", 0), ("mix_k3_ahead", 4), ("mix_tiny_weight", 7), ("r2_prior_corr", 5)]
    for name, i in picks:
        cls, params, x = made[name]
        c = cases[name]
        assert cls == c.cls and np.array_equal(x, c.x)
        got = gen.evaluate(cls, params[i % params.shape[0]], x[i])
        assert float(got["logp"]) == c.logp[i] and float(got["logp_allow"]) == c.logp_allow[i], (name, i)
        assert gen.up64([got["logp_scale"]])[0] == c.logp_scale[i] and bool(got["mask"]) == bool(c.mask[i]), (name, i)
        assert np.array_equal(np.array([float(v) for v in got["score"]]), c.score[i]), (name, i)
        assert np.array_equal(gen.up64(got["score_scale"]), c.score_scale[i]), (name, i)
        gen.cross_check(cls, params[i % params.shape[0]], x[i], got, (name, i))          # and the plain definition agrees
