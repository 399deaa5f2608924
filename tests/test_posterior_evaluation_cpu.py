"""The front of the solver's posterior evaluations (slam.PosteriorEvaluation) without a GPU: every public method goes through
`_eval_points`, the record's column-major matrix is the given values laid side by side and formed once, and the one
sample-dict checker words its refusals for samples and for a reference set."""
import contextlib
import inspect
import os
import re

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
             "posterior_modes": lambda x, smp: x.posterior_modes(smp, weights="importance"),
             "posterior_mmd_test": lambda x, smp: x.posterior_mmd_test(own, smp),
             "posterior_transport": lambda x, smp: x.posterior_transport(own, smp),
             "posterior_information": lambda x, smp: x.posterior_information(smp),
             "posterior_marginal_density": lambda x, smp: x.posterior_marginal_density(smp, curves=8),
             "posterior_trajectory_error": lambda x, smp: x.posterior_trajectory_error({X0: np.zeros(3)}, smp),
             "posterior_refine": lambda x, smp: x.posterior_refine(smp),
             "map_refine": lambda x, smp: x.map_refine(smp),
             "posterior_mcmc": lambda x, smp: x.posterior_mcmc(smp),
             "map_newton": lambda x, smp: x.map_newton(smp),
             "joint_hessian_product": lambda x, smp: x.joint_hessian_product(smp, np.zeros((7, 5)))}
    # every public method of the mixin that takes samples is listed
    takes = [k for k, f in vars(PosteriorEvaluation).items() if not k.startswith("_") and inspect.isfunction(f)
             and "samples" in inspect.signature(f).parameters]
    assert sorted(takes) == sorted(calls) and len(calls) == 19
    for solver in (s, NFiSAM()):
        for name, call in calls.items():
            for smp in (own, None) if name not in ("posterior_log_pdf", "joint_log_pdf", "joint_score",
                                                   "joint_hessian_product") else (own,):
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


@contextlib.contextmanager
def _patched(*swaps):
    """(object, name, value) triples set for the length of the block and put back after it."""
    old = [(o, k, getattr(o, k)) for o, k, _ in swaps]
    try:
        for o, k, v in swaps:
            setattr(o, k, v)
        yield
    finally:
        for o, k, v in old:
            setattr(o, k, v)


def grader_tables() -> dict:
    """Every table the two-sample graders hand to a launch, for the `_graph_solver` above, 7 own samples and a reference set of
    9 -> {name: array}.  tests/golden/make_grader_tables_fixture.py stores exactly this dict; no device is touched: the
    launches of `posterior_information` are replaced by stand-ins that record what they are given."""
    import nfisam_hip as nh
    import slam.PosteriorEvaluation as PE
    from utils import Statistics as ST
    s, X0, L1 = _graph_solver()
    rng = np.random.RandomState(0)
    own = {X0: rng.randn(7, 3), L1: rng.randn(7, 2)}
    ref = {X0: rng.randn(9, 3), L1: rng.randn(9, 2)}
    out = {}

    def same_reference(tag, Y):
        """The reference matrix depends on the order of the variables alone: stored once per order."""
        first = out.setdefault("reference/%s" % tag.rsplit("/", 1)[1], Y)
        return first.dtype == Y.dtype and np.array_equal(first, Y)

    layouts = [("%s/joint%d/extra%d/%s" % (columns, joint, extra, order), columns, joint, [(X0, L1)] if extra else None, variables)
               for columns in ("xy", "all") for joint in (True, False) for extra in (0, 1)
               for order, variables in (("default", None), ("reversed", [L1, X0]))]
    for tag, columns, joint, blocks, variables in layouts:
        nb = (1 if joint else 0) + 2 + (1 if blocks else 0)
        tables = []
        for estimator in ("mmd", "MMDb"):
            for sigma in (None, 0.7, list(np.linspace(0.5, 1.5, nb))):
                t = s._mmd_tables("posterior_mmd", ref, own, None, variables, blocks, columns, estimator, sigma, joint)
                tables.append(t["blocks"])
                for k in ("xcols", "ycols", "wrap"):
                    assert np.array_equal(out.setdefault("mmd/%s/%s" % (tag, k), t[k]), t[k])     # the same for every bandwidth
                assert same_reference(tag, t["Y"])
                assert (t["m"], t["width"]) == (9, 5)
        out["mmd/%s/blocks" % tag] = np.stack(tables)
        for axes in (True, False):
            t = s._transport_tables("posterior_transport", ref, own, None, variables, blocks, columns, 4, 0, joint, axes)
            tab, key = t["tab"], "transport/%s/axes%d/" % (tag, axes)
            for k in ("blocks", "xcols", "ycols", "dirs"):
                out[key + k] = tab[k]
            out[key + "kind"] = np.zeros(0, dtype=np.uint8) if tab["kind"] is None else tab["kind"]      # (None: no heading)
            out[key + "main_axis_at"] = np.array([tab["main"]] + [tab["axis_at"].get(b, -1) for b in range(tab["main"])])
            assert same_reference(tag, t["Y"]) and (t["m"], t["width"]) == (9, 5)

    # the reference branch of posterior_information: what its launches are handed
    seen = {}

    def entropy(St, blocks, k, flags, *a, **kw):
        seen.update(entropy_cols=np.concatenate(blocks), flags=np.asarray(flags))
        return dict(entropy=np.zeros(len(blocks)), zeros=np.zeros(len(blocks), dtype=np.int64))

    def moments(St, blocks, cols, circular, *a, **kw):
        seen.update(moment_cols=np.asarray(cols), moment_circular=np.zeros(0, np.uint8) if circular is None else circular)
        return None, None, torch.zeros(int((blocks["cov_off"] + blocks["d"].astype(np.int64) ** 2).max()), dtype=torch.float64)

    def divergence(St, Yt, pairs, *a, **kw):
        seen.update(Y=Yt, x=np.concatenate([p[0] for p in pairs]), y=np.concatenate([p[1] for p in pairs]),
                    widths=np.array([p[0].size for p in pairs]))
        return dict(divergence=np.zeros(len(pairs)))

    with _patched((PE, "_device", lambda: "cpu"), (ST, "knn_entropy_t", entropy), (nh, "sample_moments_t", moments),
                  (ST, "knn_divergence_t", divergence), (nh, "_columns", lambda A, device: A)):
        for tag, variables, reference in (("default", None, ref), ("reversed", [L1, X0], ref), ("partly", None, {L1: ref[L1]})):
            seen.clear()
            s.posterior_information(own, variables=variables, reference=reference)
            out.update({"information/%s/%s" % (tag, k): v for k, v in seen.items()})
    return {k: np.asarray(v) for k, v in out.items()}


def test_the_launches_get_the_tables_of_the_fixture(golden_dir):
    """tests/golden/grader_tables.npz was written at the commit before `_reference_front` existed (three copies of the layout):
    every table, every field of it and every dtype is the same today."""
    fx = np.load(os.path.join(golden_dir, "grader_tables.npz"))
    got = grader_tables()
    assert sorted(fx.files) == sorted(got) and len(got) > 200
    for name, a in got.items():
        want = fx[name]
        assert a.dtype == want.dtype and a.shape == want.shape, name
        for field in a.dtype.names or (None,):
            assert np.array_equal(a if field is None else a[field], want if field is None else want[field]), (name, field)
    # the reversed order is a layout of its own: a swap of xcols and ycols cannot hide behind equal arrays
    assert not np.array_equal(got["mmd/all/joint1/extra1/reversed/xcols"], got["mmd/all/joint1/extra1/reversed/ycols"])
    assert not np.array_equal(got["information/reversed/x"], got["information/reversed/y"])


def _functions_holding(pattern, *modules):
    """The functions and methods defined in `modules` whose source matches `pattern` (a nested function counts with its outer)."""
    found = []
    for mod in modules:
        scopes = [mod] + [c for c in vars(mod).values() if inspect.isclass(c) and c.__module__ == mod.__name__]
        for scope in scopes:
            for name, f in vars(scope).items():
                f = getattr(f, "__func__", getattr(f, "fget", f))          # a staticmethod's, a property's function
                if inspect.isfunction(f) and f.__module__ == mod.__name__ and re.search(pattern, inspect.getsource(f)):
                    found.append("%s.%s" % (getattr(scope, "__name__", "?"), name))
    return found


def test_no_second_copy_of_the_shared_checks_survives():
    import slam.PosteriorEvaluation as PE
    from utils import Statistics as ST
    assert len(_functions_holding(re.escape("is not in the elimination ordering"), PE)) == 1
    assert len(_functions_holding(re.escape("a block is a non-empty tuple"), PE)) == 1
    # the chord embedding: a heading's two kinds (Statistics also says `p not in (1, 2)`, which is no embedding)
    assert _functions_holding(r"\(1, 2\) if ", PE, ST) == ["utils.Statistics.transport_entries"]


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
