"""The factor densities without a GPU: `Factors.*.log_pdf` (numpy, float64) against the reference's values stored in
tests/golden/factor_density.npz (made by tests/golden/make_factor_density_fixture.py), the mixtures' log-sum-exp, an exact
multivariate normal, and the surface of the device entry (header, exports, struct size, refusals before any launch).

Bounds of the reference comparison, |ours - ref| <= RTOL |ref| + ATOL, each 16 x the largest |ours - ref| / (|ref| + 1)
measured over every value it covers (both sides are float64 evaluations at the same float32 points):
  * whole graphs (all points, all factors, per-factor terms and totals): measured 5.5e-11 (a Plaza1-ADA odometry term; the
    reference composes T_i^-1 * T_j from two rotated points ~70 m from the origin, here the difference is rotated)
    -> RTOL_G = ATOL_G = 1e-9;
  * part (a), the hand-chosen cases: measured 1.34e-8 -> RTOL_A = ATOL_A = 2.2e-7.  This is the REFERENCE's rounding error,
    not a different formula: its log map divides by cos(w) - 1 and sin(w) (geometry/TwoDimension.py:410-417), and cos(w) - 1
    has lost all but ~2 digits at the heading residuals |w| ~ 1e-7 that part (a) contains on purpose (inside the 1e-5
    branch of the Jacobian); the error of v is ~1e-16 |t| / |w|, times precision x residual (1e6 x 1e-3) = 5e-8 in the term.
    `log_pdf` uses the half-angle form (w/2) cot(w/2), which does not cancel: against the 60-digit values of the same
    cases (tests/golden/factor_exact.npz, made by tests/golden/make_factor_exact_fixture.py; held by
    tests/test_factor_exact_cpu.py and tests/test_factor_exact_gpu.py) it is within a few roundings of the value's own error
    scale where the reference is off by 3.5e-10 .. 7e-9.  Every SE(2) case with |w| > 1e-4 and every other class agrees to
    2e-9 or better (ranges, mixtures, R2 classes: 1e-15)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "factor_density.npz")
RTOL_A, ATOL_A = 2.2e-7, 2.2e-7
RTOL_G, ATOL_G = 1e-9, 1e-9
GRAPHS = {"manhattan136": "ManhattanPlaza136", "plaza1ada": "Plaza1ADA0.4EFG"}


# ---- shared with tests/test_factor_density_gpu.py ----------------------------------------------------------------------
def fixture():
    return np.load(FIXTURE)


def build_case(cls, params):
    """The factor of a part-(a) case from its stored constructor parameters (layouts: the generator's comments)."""
    X, Y = SE2Variable("X0"), SE2Variable("X1")
    L = [R2Variable("L%d" % i, VariableType.Landmark) for i in range(4)]
    p = [float(v) for v in params]
    if cls == "UnarySE2ApproximateGaussianPriorFactor":
        return F.UnarySE2ApproximateGaussianPriorFactor(X, np.array(p[:3]), np.array(p[3:]).reshape(3, 3))
    if cls == "SE2RelativeGaussianLikelihoodFactor":
        return F.SE2RelativeGaussianLikelihoodFactor(X, Y, np.array(p[:3]), covariance=np.array(p[3:]).reshape(3, 3))
    if cls == "SE2R2RangeGaussianLikelihoodFactor":
        return F.SE2R2RangeGaussianLikelihoodFactor(X, L[0], p[0], p[1])
    if cls == "R2RangeGaussianLikelihoodFactor":
        return F.R2RangeGaussianLikelihoodFactor(L[0], L[1], p[0], p[1])
    if cls == "AmbiguousDataAssociationFactor":
        k = int(p[0])
        return F.AmbiguousDataAssociationFactor(X, L[:k], np.array(p[1:1 + k]), F.SE2R2RangeGaussianLikelihoodFactor,
                                                p[1 + k], p[2 + k])
    if cls == "BinaryFactorWithNullHypo":
        return F.BinaryFactorWithNullHypo(X, L[0], np.array(p[:2]), F.SE2R2RangeGaussianLikelihoodFactor, p[2], p[3], p[4])
    if cls == "UnaryR2GaussianPriorFactor":
        return F.UnaryR2GaussianPriorFactor(L[0], np.array(p[:2]), covariance=np.array(p[2:]).reshape(2, 2))
    if cls == "R2RelativeGaussianLikelihoodFactor":
        return F.R2RelativeGaussianLikelihoodFactor(L[0], L[1], np.array(p[:2]), covariance=np.array(p[2:]).reshape(2, 2))
    if cls == "UnaryR2RangeGaussianPriorFactor":
        return F.UnaryR2RangeGaussianPriorFactor(L[0], np.array(p[:2]), p[2], p[3])
    raise KeyError(cls)


def part_a_cases(fx):
    """[(class name, factor, x float32 [n, width], reference log_pdf float64 [n])]."""
    return [(str(cls), build_case(str(cls), fx["a%03d_params" % i]), fx["a%03d_x" % i], fx["a%03d_ref" % i])
            for i, cls in enumerate(fx["a_classes"])]


def load_graph(fx, key):
    """(nodes, factors, column of every variable, x float32 [n, total], terms [n_factors, n], total [n]) of a whole graph
    of the fixture, read from tests/data with this project's parser; the fixture's variable and factor lists must match."""
    from slam.RunBatch import graph_file_parser
    nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", GRAPHS[key], "factor_graph.fg"), "fg",
                                              prior_cov_scale=0.1)
    assert [str(v.name) for v in nodes] == [str(s) for s in fx[key + "_vars"]]
    assert [f.__class__.__name__ + " " + " ".join(str(v.name) for v in f.vars) for f in factors] == \
        [str(s) for s in fx[key + "_factors"]]
    col, off = {}, 0
    for v in nodes:
        col[v] = off
        off += v.dim
    return nodes, factors, col, fx[key + "_x"], fx[key + "_terms"], fx[key + "_total"]


def factor_columns(f, col):
    return np.concatenate([np.arange(col[v], col[v] + v.dim) for v in f.vars])


def excess(got, ref, rtol, atol):
    """max of |got - ref| / (rtol |ref| + atol): <= 1 passes."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref) / (rtol * np.abs(ref) + atol))) if ref.size else 0.0


# ---- Factors.log_pdf against the reference ------------------------------------------------------------------------------------
def test_fixture_holds_no_non_finite_reference_value_and_every_class():
    fx = fixture()
    for k in fx.files:
        if fx[k].dtype.kind == "f":
            assert np.all(np.isfinite(fx[k])), k
    assert set(str(c) for c in fx["a_classes"]) == {
        "UnarySE2ApproximateGaussianPriorFactor", "SE2RelativeGaussianLikelihoodFactor", "SE2R2RangeGaussianLikelihoodFactor",
        "R2RangeGaussianLikelihoodFactor", "AmbiguousDataAssociationFactor", "BinaryFactorWithNullHypo",
        "UnaryR2GaussianPriorFactor", "UnaryR2RangeGaussianPriorFactor", "R2RelativeGaussianLikelihoodFactor"}
    assert fx["manhattan136_terms"].shape[0] == 272 and fx["plaza1ada_terms"].shape[0] == 1584
    assert fx["manhattan136_x"].dtype == np.float32 and fx["manhattan136_terms"].dtype == np.float64


def test_every_case_matches_the_reference():
    worst = 0.0
    for cls, f, x, ref in part_a_cases(fixture()):
        got = f.log_pdf(x.astype(np.float64))
        assert got.dtype == np.float64 and got.shape == ref.shape
        e = excess(got, ref, RTOL_A, ATOL_A)
        print("%-42s n = %3d   |diff| / bound = %.3g" % (cls, ref.size, e))
        worst = max(worst, e)
        if not isinstance(f, F.BinaryFactorMixture):           # (the mixtures' pdf is the plain weighted sum, see below)
            assert np.allclose(f.pdf(x.astype(np.float64)), np.exp(got), rtol=1e-12, atol=0.0), cls
    assert worst <= 1.0, worst


@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_whole_graph_terms_and_total_match_the_reference(key):
    nodes, factors, col, x, terms, total = load_graph(fixture(), key)
    x = x.astype(np.float64)
    got = np.stack([f.log_pdf(x[:, factor_columns(f, col)]) for f in factors])
    e = excess(got, terms, RTOL_G, ATOL_G)
    et = excess(got.sum(0), total, RTOL_G, ATOL_G)
    print("%s: %d factors x %d points: per-factor |diff| / bound = %.3g, total = %.3g" % (key, len(factors), x.shape[0], e, et))
    assert e <= 1.0 and et <= 1.0, (e, et)


# ---- the deliberate difference: mixtures stay finite --------------------------------------------------------------------------
def test_mixtures_far_from_every_component_are_finite_log_sum_exp():
    fx = fixture()
    seen = set()
    for cls, f, x, ref in part_a_cases(fx):
        if not isinstance(f, F.BinaryFactorMixture):
            continue
        seen.add(cls)
        x = x.astype(np.float64).copy()
        x[:, 3:] += 1.0e4                                       # every candidate ~1e4 sigma away
        with np.errstate(divide="ignore"):
            assert np.all(np.log(f.pdf(x)) == -np.inf)          # what the reference's log(sum(exp)) gives
        got = f.log_pdf(x)
        assert np.all(np.isfinite(got)) and np.all(got < -1e6)
        parts = np.stack([c.log_pdf(x[:, f.comp2idx[c]]) + np.log(w) for c, w in zip(f.components, f.weights)])
        top = parts.max(0)
        want = top + np.log(np.exp(parts - top).sum(0))
        assert np.allclose(got, want, rtol=1e-14, atol=0.0)
    assert seen == {"AmbiguousDataAssociationFactor", "BinaryFactorWithNullHypo"}


def test_mixture_pdf_is_unchanged():
    """`BinaryFactorMixture.pdf` feeds `posterior_weights`: still the plain weighted sum of the components' pdfs."""
    for cls, f, x, ref in part_a_cases(fixture()):
        if isinstance(f, F.BinaryFactorMixture):
            x = x.astype(np.float64)
            want = sum(c.pdf(x[:, f.comp2idx[c]]) * w for c, w in zip(f.components, f.weights))
            assert np.array_equal(f.pdf(x), want)


# ---- an exact case: the normaliser, without the fixture ------------------------------------------------------------------------
def test_gaussian_chain_is_the_closed_form_multivariate_normal():
    rng = np.random.RandomState(3)
    m = 5
    P = [R2Variable("P%d" % i) for i in range(m)]

    def cov():
        a = rng.randn(2, 2)
        return a @ a.T + 0.1 * np.eye(2)

    mu0, c0 = rng.randn(2), cov()
    factors = [F.UnaryR2GaussianPriorFactor(P[0], mu0, covariance=c0)]
    # joint precision J and information vector h of x = [P0 .. P4]: -0.5 x'Jx + h'x + const
    J, h = np.zeros((2 * m, 2 * m)), np.zeros(2 * m)
    J[:2, :2] += np.linalg.inv(c0)
    h[:2] += np.linalg.inv(c0) @ mu0
    for i in range(m - 1):
        obs, c = rng.randn(2) * 3, cov()
        factors.append(F.R2RelativeGaussianLikelihoodFactor(P[i], P[i + 1], obs, covariance=c))
        A = np.zeros((2, 2 * m))
        A[:, 2 * i:2 * i + 2], A[:, 2 * i + 2:2 * i + 4] = -np.eye(2), np.eye(2)
        J += A.T @ np.linalg.inv(c) @ A
        h += A.T @ np.linalg.inv(c) @ obs
    mean = np.linalg.solve(J, h)
    x = mean + rng.randn(40, 2 * m) @ np.linalg.cholesky(np.linalg.inv(J)).T * 1.5
    # a chain of conditionals with unit Jacobian: the product of the factors IS N(mean, J^-1), normaliser included
    want = -0.5 * np.einsum("ni,ij,nj->n", x - mean, J, x - mean) - 0.5 * (2 * m * np.log(2 * np.pi) - np.linalg.slogdet(J)[1])
    got = factors[0].log_pdf(x[:, :2])
    for i, f in enumerate(factors[1:]):
        got = got + f.log_pdf(x[:, 2 * i:2 * i + 4])
    assert np.allclose(got, want, rtol=1e-11, atol=1e-10), np.abs(got - want).max()


# ---- the device entry's surface --------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_exports_it(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+nfisam_factor_graph_log_density\s*\(([^)]*)\)", code)
    assert m is not None
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["terms", "n_terms", "St", "total_dim", "n", "log_p", "per_factor", "stream"]
    for name in ("PRIOR_SE2", "REL_SE2", "RANGE", "RANGE_MIX", "PRIOR_R2", "PRIOR_R2_RANGE", "REL_R2"):
        mm = re.search(r"#define\s+NFISAM_FAC_%s\s+(\d+)" % name, code)
        assert mm is not None and int(mm.group(1)) == nh.FAC_CODES[name], name
    assert "nfisam_factor_graph_log_density" in nh.EXPORTS
    nh.build()
    assert hasattr(nh.lib(), "nfisam_factor_graph_log_density")
    assert nh.lib().nfisam_abi_version() == 1600          # additive entry: the ABI version stays
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfisam_hip.h"\nint main(void) { '
                   'printf("%zu %zu %zu\\n", sizeof(nfisam_factor_term), offsetof(nfisam_factor_term, cand), '
                   'offsetof(nfisam_factor_term, p)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [C.sizeof(nh.FactorTerm), nh.FactorTerm.cand.offset, nh.FactorTerm.p.offset], sizes
    assert nh.FACTOR_DTYPE.itemsize == C.sizeof(nh.FactorTerm)
    assert [nh.FACTOR_DTYPE.fields[k][1] for k in ("code", "a", "b", "k", "cand", "p")] == \
        [getattr(nh.FactorTerm, k).offset for k in ("code", "a", "b", "k", "cand", "p")]


def test_methods_exist_and_the_parallel_solver_inherits_them():
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert callable(nh.factor_graph_log_density)
    for name in ("joint_log_pdf", "posterior_diagnostics", "map_estimate"):
        assert callable(getattr(NFiSAM, name))
        assert getattr(ParallelNFiSAM, name) is getattr(NFiSAM, name)
    assert ParallelNFiSAM.posterior_log_pdf is NFiSAM.posterior_log_pdf


def _terms(code="RANGE", a=0, b=3, k=0, cand=(0, 0, 0, 0)):
    t = np.zeros(2, dtype=nh.FACTOR_DTYPE)
    t["code"], t["a"], t["b"], t["k"], t["cand"] = nh.FAC_CODES[code], a, b, k, cand
    t["p"][:, :3] = (1.0, 4.0, -0.2)
    return t


class _Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


def test_binding_refuses_bad_tables_before_any_launch(monkeypatch):
    nh.build()
    refuse = _Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    S = np.zeros((10, 5), dtype=np.float32)                 # one pose (rows 0..2) and one landmark (rows 3..4)
    with pytest.raises(ValueError, match="out of range"):
        nh.factor_graph_log_density(_terms(b=4), S, "cpu")             # the landmark's second row would be row 5
    with pytest.raises(ValueError, match="out of range"):
        nh.factor_graph_log_density(_terms(a=-1), S, "cpu")
    with pytest.raises(ValueError, match="out of range"):
        nh.factor_graph_log_density(_terms("REL_SE2", a=0, b=3), S, "cpu")     # a pose needs three rows
    with pytest.raises(ValueError, match="out of range"):
        nh.factor_graph_log_density(_terms("RANGE_MIX", k=2, cand=(3, 4, 0, 0)), S, "cpu")
    with pytest.raises(ValueError, match="components"):
        nh.factor_graph_log_density(_terms("RANGE_MIX", k=5, cand=(3, 3, 3, 3)), S, "cpu")
    with pytest.raises(ValueError, match="components"):
        nh.factor_graph_log_density(_terms("RANGE_MIX", k=0, cand=(3, 3, 3, 3)), S, "cpu")
    bad = _terms()
    bad["code"][1] = 99
    with pytest.raises(ValueError, match="unknown factor code"):
        nh.factor_graph_log_density(bad, S, "cpu")
    with pytest.raises(ValueError, match="FACTOR_DTYPE"):
        nh.factor_graph_log_density(np.zeros(3), S, "cpu")
    with pytest.raises(ValueError, match="total_dim"):
        nh.factor_graph_log_density(_terms(), np.zeros(10, dtype=np.float32), "cpu")
    assert refuse.calls == 0


def test_pack_factor_terms_maps_records_to_rows_and_refuses_unknown_classes():
    X, L0, L1 = SE2Variable("X0"), R2Variable("L0", VariableType.Landmark), R2Variable("L1", VariableType.Landmark)
    row = {X: 4, L0: 0, L1: 2}
    fs = [F.UnarySE2ApproximateGaussianPriorFactor(X, np.array([1.0, 2.0, 0.5]), np.diag([1e-2, 1e-2, 1e-4])),
          F.SE2R2RangeGaussianLikelihoodFactor(X, L0, 3.0, 0.5),
          F.AmbiguousDataAssociationFactor(X, [L0, L1], np.array([0.3, 0.7]), F.SE2R2RangeGaussianLikelihoodFactor, 2.0, 0.25),
          F.BinaryFactorWithNullHypo(X, L1, np.array([0.9, 0.1]), F.SE2R2RangeGaussianLikelihoodFactor, 2.0, 0.25, 10.0)]
    t = nh.pack_factor_terms(fs, row)
    assert t.dtype == nh.FACTOR_DTYPE and t.shape == (4,)
    assert list(t["code"]) == [nh.FAC_CODES[c] for c in ("PRIOR_SE2", "RANGE", "RANGE_MIX", "RANGE_MIX")]
    assert list(t["a"]) == [4, 4, 4, 4] and t["b"][1] == 0
    assert list(t["k"]) == [0, 0, 2, 2]
    assert list(t["cand"][2][:2]) == [0, 2] and list(t["cand"][3][:2]) == [2, 2]        # null hypothesis: one landmark twice
    assert t["p"][3][1] == 1.0 / 0.25 ** 2 and t["p"][3][4] == 1.0 / 2.5 ** 2
    assert np.isclose(t["p"][2][2], np.log(0.3) - 0.5 * np.log(2 * np.pi * 0.25 ** 2))

    class Unknown(F.Factor):
        vars = [X]
    with pytest.raises(NotImplementedError, match="Unknown"):
        nh.pack_factor_terms(fs + [Unknown()], row)
    five = F.AmbiguousDataAssociationFactor(X, [R2Variable("M%d" % i) for i in range(5)], np.ones(5),
                                            F.SE2R2RangeGaussianLikelihoodFactor, 2.0, 0.25)
    with pytest.raises(NotImplementedError, match="at most 4"):
        nh.pack_factor_terms([five], {**row, **{v: 0 for v in five.observed_vars}})


def _fake_graph_solver(monkeypatch):
    """A solver whose graph is a pose prior and a range factor over {X0, L1}, eliminated but never trained: enough to reach
    the argument checks."""
    from slam.NFiSAM import NFiSAM
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    s.add_node(X0)
    s.add_node(L1)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    assert len(s.physical_factors) == 2
    refuse = _Refuse()
    for name in ("factor_graph_log_density", "factor_graph_log_density_t", "posterior_log_density", "posterior_log_density_t",
                 "upload"):
        monkeypatch.setattr(nh, name, refuse)
    return s, X0, L1, refuse


def test_joint_log_pdf_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    nh.build()
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().joint_log_pdf({})
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().posterior_diagnostics({})
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().map_estimate({})
    s, X0, L1, refuse = _fake_graph_solver(monkeypatch)
    good = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(ValueError, match="L1"):
        s.joint_log_pdf({X0: np.zeros((7, 3))})
    with pytest.raises(ValueError, match="ragged"):
        s.joint_log_pdf({X0: np.zeros((7, 3)), L1: np.zeros((6, 2))})
    with pytest.raises(ValueError, match="X0"):            # wrong width
        s.joint_log_pdf({X0: np.zeros((7, 2)), L1: np.zeros((7, 2))})
    with pytest.raises(RuntimeError, match="no trained model"):       # diagnostics need log q: a trained tree
        s.posterior_diagnostics(good)

    class Unknown(F.Factor):
        vars = [X0]
    s.physical_factor_graph.add_factor(Unknown())
    with pytest.raises(NotImplementedError, match="Unknown"):
        s.joint_log_pdf(good)
    assert refuse.calls == 0
