"""The front of the solver's posterior evaluations (slam.PosteriorEvaluation) without a GPU: every public method goes through
`_eval_points`, the record's column-major matrix is the given values laid side by side and formed once, and the one
sample-dict checker words its refusals for samples and for a reference set."""
import numpy as np
import pytest
import torch

from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType


class ThroughTheFront(Exception):
    pass


def _graph_solver():
    from slam.NFiSAM import NFiSAM
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    s.add_node(X0)
    s.add_node(L1)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    return s, X0, L1


def test_every_public_evaluation_goes_through_the_one_front(monkeypatch):
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    from slam.PosteriorEvaluation import PosteriorEvaluation
    assert issubclass(NFiSAM, PosteriorEvaluation) and ParallelNFiSAM.posterior_summary is NFiSAM.posterior_summary
    for name in ("_post_columns", "_posterior_table", "_joint_terms", "posterior_launch"):
        assert callable(getattr(NFiSAM, name))
    seen = []

    def front(self, what, samples, *a, **k):
        seen.append(what)
        raise ThroughTheFront(what)
    monkeypatch.setattr(NFiSAM, "_eval_points", front)
    s, X0, L1 = _graph_solver()
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    calls = {"posterior_log_pdf": lambda x, smp: x.posterior_log_pdf(smp, per_clique=True),
             "joint_log_pdf": lambda x, smp: x.joint_log_pdf(smp, per_factor=True),
             "posterior_diagnostics": lambda x, smp: x.posterior_diagnostics(smp),
             "map_estimate": lambda x, smp: x.map_estimate(smp),
             "joint_score": lambda x, smp: x.joint_score(smp),
             "posterior_ksd": lambda x, smp: x.posterior_ksd(smp, nboot=3, seed=0),
             "posterior_mmd": lambda x, smp: x.posterior_mmd(own, smp, estimator="MMDu2", columns="all"),
             "posterior_summary": lambda x, smp: x.posterior_summary(smp, weights="importance"),
             "posterior_modes": lambda x, smp: x.posterior_modes(smp, weights="importance")}
    for solver in (s, NFiSAM()):
        for name, call in calls.items():
            for smp in (own, None) if name not in ("posterior_log_pdf", "joint_log_pdf", "joint_score") else (own,):
                seen.clear()
                with pytest.raises(ThroughTheFront):
                    call(solver, smp)
                assert seen == ["posterior_diagnostics" if name == "map_estimate" else name]
    # what is pinned to fire before the front still does
    with pytest.raises(ValueError, match="estimator"):
        s.posterior_mmd(own, own, estimator="MMD")
    with pytest.raises(ValueError, match="columns"):
        s.posterior_mmd(own, own, columns="xyz")
    with pytest.raises(ValueError, match="'importance'"):
        s.posterior_summary(own, weights="uniform")
    with pytest.raises(ValueError, match="'importance'"):
        s.posterior_modes(own, weights="uniform")


def test_the_record_lays_the_values_out_column_major_and_once():
    from slam.PosteriorEvaluation import EvalPoints
    s, X0, L1 = _graph_solver()
    rng = np.random.RandomState(0)
    a, b = rng.randn(5, 3), rng.randn(5, 2).astype(np.float32)
    pcol = {L1: 0, X0: 3}                                   # a layout with a gap: column 2 belongs to nobody
    want = np.zeros((6, 5), dtype=np.float32)
    want[3:6], want[0:2] = a.T, b.T
    for values in ({X0: a, L1: b}, {X0: torch.from_numpy(a), L1: torch.from_numpy(b)}, {X0: torch.from_numpy(a), L1: b}):
        pts = EvalPoints(s, values, 5, pcol, 6, dict(device="cpu"))
        St = pts.St
        assert St.dtype == torch.float32 and St.is_contiguous() and np.array_equal(St.numpy(), want)
        assert pts.St is St and pts.device == torch.device("cpu")
    none = EvalPoints(s, {X0: a[:0], L1: b[:0]}, 0, pcol, 6, dict(device="cpu"))
    assert tuple(none.St.shape) == (6, 0)


def test_one_checker_words_samples_and_reference():
    from slam.PosteriorEvaluation import _REFERENCE_NOUNS
    s, X0, L1 = _graph_solver()
    good = {X0: np.zeros((7, 3)), L1: torch.zeros(7, 2)}
    values, n = s._check_points(good, "f")
    assert n == 7 and list(values) == list(s._elimination_ordering) and values[L1] is good[L1]
    ref, m = s._check_points(good, "f", [L1], _REFERENCE_NOUNS, host=True)
    assert m == 7 and list(ref) == [L1] and isinstance(ref[L1], np.ndarray)
    for kw, bad, text in (({}, {X0: good[X0]}, "f: samples lack variable L1"),
                          ({}, {X0: np.zeros((7, 2)), L1: good[L1]}, r"f: samples of X0 must be \[n, 3\], got \(7, 2\)"),
                          ({}, {X0: np.zeros((6, 3)), L1: np.zeros((7, 2))}, "f: ragged samples: .* has [67] rows, the others [67]"),
                          (dict(variables=[X0, L1], nouns=_REFERENCE_NOUNS, host=True), {X0: good[X0]},
                           "f: the reference lacks variable L1"),
                          (dict(variables=[X0], nouns=_REFERENCE_NOUNS, host=True), {X0: np.zeros((7, 2))},
                           r"f: reference samples of X0 must be \[m, 3\], got \(7, 2\)"),
                          (dict(variables=[X0, L1], nouns=_REFERENCE_NOUNS, host=True), {X0: np.zeros((9, 3)), L1: np.zeros((8, 2))},
                           "f: ragged reference: L1 has 8 rows, the others 9")):
        with pytest.raises(ValueError, match=text):
            s._check_points(bad, "f", **kw)
