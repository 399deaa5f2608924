"""The factor scores without a GPU: `Factors.*.grad_x_log_pdf` (numpy, float64) against tests/golden/factor_score.npz (made
by tests/golden/make_factor_score_fixture.py from the reference's own `grad_x_log_pdf`, or Richardson differences of its
`log_pdf` for the three R2 classes behind the TransportMaps stub), the gather lists of `pack_score_gather`, and the refusals
of the score binding before any launch.

Bounds, |ours - ref| <= TOL (|ref| + 1) on the rows the fixture's masks cover, each 16 x the largest
|ours - ref| / (|ref| + 1) measured over the values it covers (both sides float64 at the same float32 points):
  * part (a), every value:  measured 0.301  -> TOL_A = 4.82;   whole graphs, every value:  measured 1.95e-3 -> TOL_G = 3.12e-2.
    These two are the REFERENCE's error, not this code's.  Its SE(2) `grad_x_log_pdf` builds d Log / d theta from
    logmap / w + (w / 2) x / (cos w - 1) (geometry/TwoDimension.py:431-435): two terms of size |t| / w that cancel, with
    cos w - 1 correct to 1e-16 / w^2 relative -- an O(1) error at the |w| ~ 1e-5 rows part (a) holds on purpose -- and it
    switches to a first-order form below 1e-5.  The exact yardstick of these rows is tests/golden/factor_exact.npz (60-digit
    values and gradients of the smooth density, made by tests/golden/make_factor_exact_fixture.py): `grad_x_log_pdf` is held
    to it, every SE(2) value of part (a) included, within 256 roundings of the value's own error scale by
    tests/test_factor_exact_cpu.py (the device: tests/test_factor_exact_gpu.py), where the reference is off by up to 0.43.  The
    finite difference the fixture also stores agrees with this code, not with the reference's analytic value, on those rows.
  * so the same comparison is also made where the reference does not cancel, with the bound the same rule gives there:
      ranges and mixtures (reference analytic)                   measured 3.8e-16  -> TOL_EXACT = 6.1e-15
      the three R2 classes (Richardson differences, step 1e-3 sigma) measured 7.4e-11  -> TOL_FD = 1.2e-9
      SE(2) rows with a heading residual |w| >= 1e-3              measured 4.5e-7   -> TOL_SE2 = 7.2e-6
On the masked rows (a range of exactly 0; nothing else needed masking) the score must be finite, and 0 at range 0."""
import os

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from geometry.TwoDimension import wrap_pi
from slam.Variables import R2Variable, SE2Variable, VariableType
from test_factor_density_cpu import GRAPHS, factor_columns, fixture, load_graph, part_a_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "factor_score.npz")
MEASURED = {"part_a": 0.301, "graphs": 1.95e-3, "exact": 3.8e-16, "fd": 7.4e-11, "se2": 4.5e-7}
TOL_A, TOL_G = 16 * MEASURED["part_a"], 16 * MEASURED["graphs"]
TOL_EXACT, TOL_FD, TOL_SE2 = 16 * MEASURED["exact"], 16 * MEASURED["fd"], 16 * MEASURED["se2"]
SE2_CLASSES = ("UnarySE2ApproximateGaussianPriorFactor", "SE2RelativeGaussianLikelihoodFactor")


# ---- shared with tests/test_factor_score_gpu.py and tests/test_sample_ksd_*.py -----------------------------------------------
def score_fixture():
    return np.load(FIXTURE)


def deviation(got, ref):
    """largest |got - ref| / (|ref| + 1)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + 1.0))) if ref.size else 0.0


def part_a_scores(fs=None):
    """[(class name, factor, x float32 [n, width], reference score [n, width], mask [n], group)]: group is "se2", "exact"
    (the reference's analytic value of a class without cancellation) or "fd" (Richardson differences)."""
    fs = score_fixture() if fs is None else fs
    out = []
    for i, (cls, f, x, _) in enumerate(part_a_cases(fixture())):
        group = "se2" if cls in SE2_CLASSES else ("exact" if bool(fs["a%03d_analytic" % i]) else "fd")
        out.append((cls, f, x, fs["a%03d_ref" % i], fs["a%03d_mask" % i], group))
    return out


def heading_residual(f, x):
    """w of an SE(2) case's rows (float64)."""
    x = x.astype(np.float64)
    if isinstance(f, F.UnarySE2ApproximateGaussianPriorFactor):
        return wrap_pi(x[:, 2] - f.observation[2])
    return wrap_pi(x[:, 5] - x[:, 2] - f.observation[2])


def host_joint_score(factors, col, x):
    """sum over the factors of `grad_x_log_pdf`, added per column in factor order: [n, total] float64."""
    x = np.asarray(x, dtype=np.float64)
    G = np.zeros_like(x)
    for f in factors:
        c = factor_columns(f, col)
        G[:, c] += f.grad_x_log_pdf(x[:, c])
    return G


def graph_scores(key, fs=None):
    """(factors, col, x float32 [n, total], reference score [n, total]) of a whole graph at the fixture's rows."""
    fs = score_fixture() if fs is None else fs
    nodes, factors, col, x, _, _ = load_graph(fixture(), key)
    return factors, col, x[fs[key + "_rows"]], fs[key + "_score"]


def ksd_graph(truth):
    """The 13-dimensional graph of fixture part (c) with this project's classes -> (variables, factors)."""
    P = [SE2Variable("X%d" % i) for i in range(3)]
    M = [R2Variable("L%d" % i, VariableType.Landmark) for i in range(2)]
    odo = np.diag([0.04, 0.04, 0.01])
    factors = [F.UnarySE2ApproximateGaussianPriorFactor(P[0], np.zeros(3), np.diag([0.01, 0.01, 0.0025])),
               F.SE2RelativeGaussianLikelihoodFactor(P[0], P[1], np.array([2.0, 0.0, 0.5]), covariance=odo),
               F.SE2RelativeGaussianLikelihoodFactor(P[1], P[2], np.array([1.8, 0.16, 0.7]), covariance=odo)]

    def dist(a, b):
        return float(np.sqrt(((truth[a:a + 2] - truth[b:b + 2]) ** 2).sum()))
    for pose, lm in ((0, 0), (1, 0), (1, 1), (2, 1)):
        factors.append(F.SE2R2RangeGaussianLikelihoodFactor(P[pose], M[lm], dist(3 * pose, 9 + 2 * lm), 0.3))
    factors.append(F.AmbiguousDataAssociationFactor(P[2], M, np.array([0.5, 0.5]), F.SE2R2RangeGaussianLikelihoodFactor,
                                                    dist(6, 9), 0.3))
    return P + M, factors


# ---- Factors.grad_x_log_pdf against the fixture ------------------------------------------------------------------------------------
def test_fixture_masks_drop_at_most_five_percent_and_only_where_the_reference_is_undefined():
    fs = score_fixture()
    for i, (cls, f, x, ref, mask, group) in enumerate(part_a_scores(fs)):
        assert ref.shape == x.shape and mask.shape == (x.shape[0],) and fs["a%03d_fd" % i].shape == x.shape
        assert np.all(np.isfinite(ref)) and np.all(np.isfinite(fs["a%03d_fd" % i]))
        assert (~mask).sum() <= 0.05 * mask.size, cls
    assert fs["manhattan136_score"].shape == (48, 416) and fs["plaza1ada_score"].shape[1] == 2342


def test_every_case_matches_the_fixture():
    worst = dict(part_a=0.0, exact=0.0, fd=0.0, se2=0.0)
    for cls, f, x, ref, mask, group in part_a_scores():
        got = f.grad_x_log_pdf(x.astype(np.float64))
        assert got.dtype == np.float64 and got.shape == ref.shape and np.all(np.isfinite(got)), cls
        d_all = deviation(got[mask], ref[mask])
        if group == "se2":
            big = np.abs(heading_residual(f, x)) >= 1e-3
            d = deviation(got[big], ref[big])
        else:
            d = d_all
        print("%-42s %-5s rows %2d   |ours - ref| / (|ref| + 1): all %.3g, group %.3g" % (cls, group, ref.shape[0], d_all, d))
        worst["part_a"], worst[group] = max(worst["part_a"], d_all), max(worst[group], d)
    print("measured:", worst)
    assert worst["part_a"] <= TOL_A and worst["exact"] <= TOL_EXACT and worst["fd"] <= TOL_FD and worst["se2"] <= TOL_SE2, worst


def test_masked_rows_are_finite_and_zero_at_range_zero():
    seen = 0
    for cls, f, x, ref, mask, group in part_a_scores():
        if mask.all():
            continue
        got = f.grad_x_log_pdf(x.astype(np.float64))[~mask]
        seen += got.shape[0]
        assert np.all(np.isfinite(got)), cls
        if not isinstance(f, F.BinaryFactorMixture) or cls == "BinaryFactorWithNullHypo":
            assert np.all(got == 0.0), cls            # a range of exactly 0 (both components of the null-hypothesis factor)
    assert seen >= 10


@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_whole_graph_scores_match_the_fixture(key):
    factors, col, x, ref = graph_scores(key)
    d = deviation(host_joint_score(factors, col, x), ref)
    print("%s: %d factors x %d points: |ours - ref| / (|ref| + 1) = %.3g" % (key, len(factors), x.shape[0], d))
    assert d <= TOL_G, d


def test_the_ksd_graph_score_matches_the_fixture():
    fs = score_fixture()
    variables, factors = ksd_graph(fs["ksd_truth"])
    assert [f.__class__.__name__ + " " + " ".join(str(v.name) for v in f.vars) for f in factors] == \
        [str(s) for s in fs["ksd_factors"]]
    col, off = {}, 0
    for v in variables:
        col[v] = off
        off += v.dim
    d = deviation(host_joint_score(factors, col, fs["ksd_samples"]), fs["ksd_score"])
    print("ksd graph: |ours - ref| / (|ref| + 1) = %.3g" % d)
    assert d <= TOL_G, d


def test_mixture_scores_far_from_every_component_are_finite_softmax_weights():
    for cls, f, x, ref, mask, group in part_a_scores():
        if not isinstance(f, F.BinaryFactorMixture):
            continue
        x = x.astype(np.float64).copy()
        x[:, 3:] += 1.0e4
        assert np.all(f.pdf(x) == 0.0)                       # where the reference divides by zero
        got = f.grad_x_log_pdf(x)
        assert np.all(np.isfinite(got)) and np.abs(got).max() > 10.0
        terms = np.stack([c.log_pdf(x[:, f.comp2idx[c]]) + np.log(w) for c, w in zip(f.components, f.weights)])
        r = np.exp(terms - terms.max(0))
        r /= r.sum(0)
        want = np.zeros_like(x)
        for k, c in enumerate(f.components):
            want[:, f.comp2idx[c]] += r[k][:, None] * c.grad_x_log_pdf(x[:, f.comp2idx[c]])
        assert np.allclose(got, want, rtol=1e-14, atol=0.0)


def test_small_angle_series_joins_the_plain_form():
    """Either side of the switch |w / 2| = 0.1 the two forms agree to the two digits the threshold was chosen for, and the
    series has no plateau at the value formula's own branches (|w| < 1e-10, |w| < 1e-5)."""
    w = np.array([np.nextafter(0.2, 0.0), 0.2])                      # the last series argument, the first plain one
    a, da, dl = F._log_map_terms(w)
    for v in (a, da, dl):
        assert abs(v[0] - v[1]) <= 1e-13 * abs(v[1])
    a, da, dl = F._log_map_terms(np.array([0.0, 1e-12, 3e-6, 1e-5, 1e-3]))
    h = 0.5 * np.array([0.0, 1e-12, 3e-6, 1e-5, 1e-3])
    assert np.allclose(da, -h / 3, rtol=1e-6, atol=0.0) and np.allclose(dl, h / 3, rtol=1e-6, atol=0.0) and a[0] == 1.0


# ---- the gather lists ------------------------------------------------------------------------------------------------------------------
def test_pack_score_gather_lists_every_slot_once_in_table_order():
    X = SE2Variable("X0")
    L = [R2Variable("L%d" % i, VariableType.Landmark) for i in range(3)]
    factors = [F.SE2R2RangeGaussianLikelihoodFactor(X, L[1], 4.0, 0.5),
               F.BinaryFactorWithNullHypo(X, L[0], np.array([0.9, 0.1]), F.SE2R2RangeGaussianLikelihoodFactor, 8.0, 0.5, 10.0),
               F.UnarySE2ApproximateGaussianPriorFactor(X, np.zeros(3), np.eye(3)),
               F.AmbiguousDataAssociationFactor(X, L, np.ones(3), F.SE2R2RangeGaussianLikelihoodFactor, 3.0, 0.4),
               F.UnaryR2GaussianPriorFactor(L[1], np.zeros(2), covariance=np.eye(2))]
    rows = {X: 2, L[0]: 5, L[1]: 9, L[2]: 7}                           # rows not in table order, row 0, 1 and 11 unused
    terms = nh.pack_factor_terms(factors, rows)
    g = nh.pack_score_gather(terms, 12)
    assert list(g["slot_off"]) == [0, 4, 10, 13, 21] and g["n_slots"] == 23
    assert g["row_off"].dtype == g["row_slot"].dtype == g["slot_off"].dtype == np.int32
    assert g["row_off"].shape == (13,) and g["row_off"][0] == 0 and g["row_off"][-1] == 23
    assert sorted(g["row_slot"]) == list(range(23))                    # every slot exactly once
    per_row = [list(g["row_slot"][g["row_off"][r]:g["row_off"][r + 1]]) for r in range(12)]
    assert all(p == sorted(p) for p in per_row)                        # table order within a row
    assert per_row[0] == per_row[1] == per_row[11] == [] and per_row[4] == [12]
    assert per_row[2] == [0, 4, 10, 13] and per_row[3] == [1, 5, 11, 14]
    assert per_row[5] == [6, 8, 15] and per_row[6] == [7, 9, 16]       # the twice-listed candidate lands in the same rows
    assert per_row[9] == [2, 17, 21] and per_row[7] == [19]
    empty = nh.pack_score_gather(terms[:0], 5)
    assert empty["n_slots"] == 0 and not empty["row_off"].any()


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
def test_score_binding_refuses_bad_input_with_no_device():
    X = SE2Variable("X0")
    L0 = R2Variable("L0", VariableType.Landmark)
    terms = nh.pack_factor_terms([F.SE2R2RangeGaussianLikelihoodFactor(X, L0, 4.0, 0.5)], {X: 0, L0: 3})
    S = np.zeros((4, 5), dtype=np.float32)
    with pytest.raises(ValueError, match="out of range"):
        nh.factor_graph_score(terms, S[:, :4], "cuda")
    with pytest.raises(ValueError, match="out of range"):
        nh.pack_score_gather(terms, 4)
    bad = terms.copy()
    bad["code"] = 9
    with pytest.raises(ValueError, match="unknown factor code"):
        nh.factor_graph_score(bad, S, "cuda")
    mix = terms.copy()
    mix["code"], mix["k"] = nh.FAC_CODES["RANGE_MIX"], 5
    with pytest.raises(ValueError, match="1..4 components"):
        nh.pack_score_gather(mix, 5)
    with pytest.raises(ValueError, match="S must be"):
        nh.factor_graph_score(terms, np.zeros(5, dtype=np.float32), "cuda")
    with pytest.raises(ValueError, match="FACTOR_DTYPE"):
        nh.factor_graph_score(np.zeros(3), S, "cuda")
    with pytest.raises(ValueError, match="contiguous float32"):
        nh.factor_graph_score_t(terms, torch.zeros(5, 4, dtype=torch.float64), "cuda")
    with pytest.raises(ValueError, match="another table"):
        nh.factor_graph_score_t(terms, torch.zeros(5, 4), "cuda", gather=nh.pack_score_gather(terms, 6))

    class Opaque(F.Factor):
        vars = [X]
    with pytest.raises(NotImplementedError, match="Opaque"):
        nh.pack_factor_terms([Opaque()], {X: 0})


def test_the_new_entries_are_declared_with_the_reference_lines_they_replace():
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    for name in ("nfisam_factor_graph_score", "nfisam_factor_graph_score_scratch_count", "nfisam_sample_ksd",
                 "nfisam_sample_ksd_scratch_count"):
        assert name in nh.EXPORTS and name + "(" in hdr
    assert "sampler_utils.py:100-113" in hdr and "Statistics.py:216-245" in hdr
    lib = nh.lib()
    assert lib.nfisam_factor_graph_score_scratch_count(23, 130) == 23 * 130
    assert lib.nfisam_sample_ksd_scratch_count(130) == 3 * 3 * 64 and lib.nfisam_sample_ksd_scratch_count(0) == 0
    assert lib.nfisam_sample_ksd_scratch_count(65535 * 64 + 1) == 0
