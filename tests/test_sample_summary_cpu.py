"""The sample summaries without a GPU: the surface of the two device entries (header, exports, struct size), their host-side
refusals and those of the binding and of `NFiSAM.posterior_summary` before anything is launched, and the host functions
`rmse`, `translation_distance`, `geodesic_distance` of `utils.Statistics` against the reference's own values
(tests/golden/sample_summary.npz, written by tests/golden/make_sample_summary_fixture.py).

The float64 oracle of tests/test_sample_summary_gpu.py lives here (`oracle_moments`, `oracle_quantiles`): the float32 points
cast to float64, elementwise parts in numpy float64, EVERY sum by math.fsum, which rounds the exact sum once -- so a
comparison bounds the device's error alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, Variable, VariableType
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- shared with tests/test_sample_summary_gpu.py -----------------------------------------------------------------------------
def wrap_pi(t):
    return (t + np.pi) % (2.0 * np.pi) - np.pi


def oracle_moments(x, cols, circular=None, weights=None):
    """One block: (mean [d], resultant [d] (NaN where not circular), cov [d, d], s [d] = max_i |r_e,i|) of the columns `cols`
    of x.  The Euclidean mean is x_0 + fsum(w (x - x_0)) / fsum(w): x - x_0 is exact in float64 for float32 data, so this is
    the weighted mean with one rounding less than fsum(w x) / fsum(w), and a constant column has mean x_0 exactly.  Likewise
    the circular mean is x_0 + atan2(S', C') of the sums of sin / cos (x - x_0): the direction and length of atan2(S, C)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)[:, list(cols)]
    n, d = x.shape
    circ = np.zeros(d, dtype=bool) if circular is None else np.asarray(circular, dtype=bool)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    W = math.fsum(w)
    mean, res = np.zeros(d), np.full(d, np.nan)
    r = np.zeros_like(x)
    for e in range(d):
        if circ[e]:
            a = x[:, e] - x[0, e]
            c, s = math.fsum(w * np.cos(a)) / W, math.fsum(w * np.sin(a)) / W
            m = x[0, e] + math.atan2(s, c)
            mean[e], res[e] = (m if -np.pi <= m < np.pi else wrap_pi(m)), math.hypot(c, s)
            r[:, e] = wrap_pi(x[:, e] - mean[e])
        else:
            mean[e] = x[0, e] + math.fsum(w * (x[:, e] - x[0, e])) / W
            r[:, e] = x[:, e] - mean[e]
    cov = np.array([[math.fsum(w * r[:, e] * r[:, f]) / W for f in range(d)] for e in range(d)])
    return mean, res, cov, np.abs(r).max(axis=0)


def oracle_quantiles(x, col, probs, circular=False, center=0.0):
    """(np.quantile of the float64 keys of one column [n_probs], the sorted keys): x, or wrap_pi(x - center) for an angle,
    which reports center + quantile unwrapped."""
    k = np.asarray(x, dtype=np.float32).astype(np.float64)[:, col]
    if circular:
        k = wrap_pi(k - center)
    s = np.sort(k)
    q = np.quantile(s, np.asarray(probs, dtype=np.float64))
    return (q + center if circular else q), s


class Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_library_exports_both_entries_and_the_abi_version_stays():
    nh.build()
    lib = nh.lib()
    for name in ("nfisam_sample_moments", "nfisam_sample_quantiles"):
        assert name in nh.EXPORTS and hasattr(lib, name), name
    assert lib.nfisam_abi_version() == 1600
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    assert "int nfisam_sample_moments(" in hdr and "int nfisam_sample_quantiles(" in hdr
    assert "#define NFISAM_MOMENTS_MAX_D  16" in hdr and "#define NFISAM_QUANTILE_MAX_N 16384" in hdr
    assert "Statistics.py:151-171" in hdr and "mean squared WRAPPED deviation" in hdr
    assert nh.MOMENTS_MAX_D == 16 and nh.QUANTILE_MAX_N == 16384
    for f in (nh.sample_moments, nh.sample_moments_t, nh.sample_quantiles, nh.sample_quantiles_t, ST.sample_moments,
              ST.sample_quantiles, ST.sample_mean, ST.rmse, ST.translation_distance, ST.geodesic_distance):
        assert callable(f)


def test_struct_size_is_16_and_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfisam_hip.h"\nint main(void) { '
                   'printf("%zu %zu %zu %d %d\\n", sizeof(nfisam_moment_block), offsetof(nfisam_moment_block, d), '
                   'offsetof(nfisam_moment_block, cov_off), NFISAM_MOMENTS_MAX_D, NFISAM_QUANTILE_MAX_N); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [16, 4, 8, 16, 16384]
    assert sizes[:3] == [C.sizeof(nh.MomentBlock), nh.MomentBlock.d.offset, nh.MomentBlock.cov_off.offset]
    assert nh.MOMENT_BLOCK_DTYPE.itemsize == 16
    assert [nh.MOMENT_BLOCK_DTYPE.fields[k][1] for k in ("col_off", "d", "cov_off")] == [0, 4, 8]


def test_host_side_refusals_of_the_c_entries():
    """Both entries refuse bad arguments on the host, before they touch the device (the pointers below are never
    dereferenced: they are not device memory)."""
    nh.build()
    lib = nh.lib()
    blocks = nh.pack_moment_blocks([2, 3])
    fake = C.c_void_p(4096)
    ll = C.c_longlong

    def moments(Xt=fake, n=5, blk=blocks, blk_dev=fake, nb=2, cols=fake, ne=5, mean=fake, res=fake, cov=fake, count=13, rows=4):
        return lib.nfisam_sample_moments(Xt, rows, n, None if blk is None else blk.ctypes.data_as(C.c_void_p), blk_dev, nb, cols,
                                         ne, None, None, mean, res, cov, ll(count), None)
    for kw in (dict(Xt=None), dict(blk=None), dict(blk_dev=None), dict(cols=None), dict(mean=None), dict(res=None), dict(cov=None),
               dict(n=0), dict(n=-3), dict(nb=0), dict(nb=65536), dict(ne=0), dict(rows=0), dict(count=0), dict(count=12)):
        assert moments(**kw) == nh.ERR_ARG, kw
    for d in (0, -1, 17):
        bad = blocks.copy()
        bad["d"][1] = d
        assert moments(blk=bad) == nh.ERR_ARG, d
    bad = blocks.copy()
    bad["cov_off"][0] = -1
    assert moments(blk=bad) == nh.ERR_ARG
    many = nh.pack_moment_blocks(np.ones(65536, dtype=np.int64))
    assert moments(blk=many, nb=65536, ne=65536, count=65536) == nh.ERR_ARG

    def quantiles(Xt=fake, n=5, cols=fake, ne=2, probs=(0.5,), probs_dev=fake, np_=None, out=fake, rows=4):
        p = None if probs is None else (C.c_double * len(probs))(*probs)
        return lib.nfisam_sample_quantiles(Xt, rows, n, cols, ne, None, None, p, probs_dev,
                                           (len(probs) if probs is not None else 1) if np_ is None else np_, out, None)
    for kw in (dict(Xt=None), dict(cols=None), dict(probs=None), dict(probs_dev=None), dict(out=None), dict(n=0), dict(ne=0),
               dict(rows=0), dict(np_=0), dict(np_=-1), dict(n=16385), dict(n=1 << 20), dict(probs=(0.5, 1.0000001)),
               dict(probs=(-1e-9,)), dict(probs=(float("nan"),))):
        assert quantiles(**kw) == nh.ERR_ARG, kw


def test_check_moment_blocks_refuses_bad_offsets_widths_and_rows():
    t = nh.pack_moment_blocks([2, 3, 1])
    assert list(t["col_off"]) == [0, 2, 5] and list(t["d"]) == [2, 3, 1] and list(t["cov_off"]) == [0, 4, 13]
    cols = [0, 1, 2, 3, 4, 4]
    nh.check_moment_blocks(t, cols, 5)
    nh.check_moment_blocks(t, cols, 5, circular=np.zeros(6, dtype=np.uint8))
    for field, value, match in (("col_off", 4, "leave"), ("col_off", -1, "leave"), ("d", 0, "width"), ("d", 17, "width"),
                                ("d", 5, "leave"), ("cov_off", -1, "matrix"), ("cov_off", 6, "matrix")):
        bad = t.copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match=match):
            nh.check_moment_blocks(bad, cols, 5, cov_count=14)
    with pytest.raises(ValueError, match="cols"):
        nh.check_moment_blocks(t, cols, 4)
    with pytest.raises(ValueError, match="cols"):
        nh.check_moment_blocks(t, [0, 1, -1, 3, 4, 4], 5)
    with pytest.raises(ValueError, match="circular"):
        nh.check_moment_blocks(t, cols, 5, circular=np.zeros(5))
    with pytest.raises(ValueError, match="MOMENT_BLOCK_DTYPE"):
        nh.check_moment_blocks(np.zeros(2), cols, 5)
    with pytest.raises(ValueError, match="blocks"):
        nh.check_moment_blocks(t[:0], cols, 5)
    with pytest.raises(ValueError, match="blocks"):
        nh.check_moment_blocks(nh.pack_moment_blocks(np.ones(65536, dtype=np.int64)), np.zeros(65536, dtype=np.int64), 5)


def test_cpu_tensors_and_bad_arguments_are_refused_before_any_launch(monkeypatch):
    refuse = Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    t = nh.pack_moment_blocks([2])
    X = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_moments(X, t, [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_moments(X.numpy(), t, [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_moments_t(X.t().contiguous(), t, [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_quantiles(X, [0, 1], [0.5])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_quantiles_t(X.t().contiguous(), [0, 1], [0.5])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.sample_moments(X, [[0, 1]])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.sample_quantiles(X, [0.5])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.sample_mean(X, [SE2Variable("X0")])
    x = X.numpy()                                                         # refused before the device is asked for
    with pytest.raises(ValueError, match="cols"):
        nh.sample_moments(x, t, [0, 3], device="cuda")
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        nh.sample_moments(np.zeros(5, dtype=np.float32), t, [0, 1], device="cuda")
    with pytest.raises(ValueError, match="no points"):
        nh.sample_moments(x[:0], t, [0, 1], device="cuda")
    for w, match in ((np.ones(4), r"\[n\]"), (-np.ones(5), "non-negative"), (np.zeros(5), "all zero"),
                     (np.array([1, np.nan, 1, 1, 1.0]), "finite"), (np.array([1, np.inf, 1, 1, 1.0]), "finite")):
        with pytest.raises(ValueError, match=match):
            nh.sample_moments(x, t, [0, 1], weights=w, device="cuda")
    with pytest.raises(ValueError, match="outside"):
        nh.sample_quantiles(x, [0, 1], [0.5, 1.5], device="cuda")
    with pytest.raises(ValueError, match="probs"):
        nh.sample_quantiles(x, [0, 1], [], device="cuda")
    with pytest.raises(ValueError, match="cols"):
        nh.sample_quantiles(x, [0, 3], [0.5], device="cuda")
    with pytest.raises(ValueError, match="16384"):
        nh.sample_quantiles(np.zeros((16385, 1), dtype=np.float32), [0], [0.5], device="cuda")
    with pytest.raises(ValueError, match="center"):
        nh.sample_quantiles(x, [0, 1], [0.5], circular=[0, 1], center=[0.0], device="cuda")
    with pytest.raises(ValueError, match="at most 16"):
        ST.sample_moments(np.zeros((5, 17)), [list(range(17))], device="cuda")
    with pytest.raises(ValueError, match="outside"):
        ST.sample_moments(x, [[0, 3]], device="cuda")
    with pytest.raises(ValueError, match="block 1"):
        ST.sample_moments(x, [[0], []], device="cuda")
    with pytest.raises(ValueError, match="circular"):
        ST.sample_moments(x, [[0]], circular=[True], device="cuda")
    with pytest.raises(ValueError, match="circular"):
        ST.sample_quantiles(x, [0.5], circular=[True], device="cuda")
    assert refuse.calls == 0


# ---- the solver -------------------------------------------------------------------------------------------------------------
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
    refuse = Refuse()
    for name in ("sample_moments", "sample_moments_t", "sample_quantiles", "sample_quantiles_t", "posterior_walk_raw", "upload",
                 "posterior_log_density", "posterior_log_density_t", "factor_graph_log_density", "factor_graph_log_density_t"):
        monkeypatch.setattr(nh, name, refuse)
    return s, X0, L1, refuse


def test_posterior_summary_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_summary is NFiSAM.posterior_summary
    nh.build()
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().posterior_summary()
    s, X0, L1, refuse = _fake_graph_solver(monkeypatch)
    X9 = SE2Variable("X9")
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):      # a draw needs a trained tree
        s.posterior_summary()
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):      # and so does log q of given points
        s.posterior_summary(own, weights="importance")
    with pytest.raises(ValueError, match="'importance'"):
        s.posterior_summary(own, weights="uniform")
    with pytest.raises(ValueError, match="X9 is not in the elimination ordering"):
        s.posterior_summary(own, variables=[X0, X9])
    with pytest.raises(ValueError, match="X9 is not in the elimination ordering"):
        s.posterior_summary(own, pairs=[(X0, X9)])
    with pytest.raises(ValueError, match="pair"):
        s.posterior_summary(own, pairs=[(X0, L1, X0)])
    with pytest.raises(ValueError, match="no variable"):
        s.posterior_summary(own, variables=[])
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_summary({X0: own[X0]})
    with pytest.raises(ValueError, match="ragged samples"):
        s.posterior_summary({X0: np.zeros((7, 3)), L1: np.zeros((6, 2))})
    with pytest.raises(ValueError, match="samples of L1"):
        s.posterior_summary({X0: np.zeros((7, 3)), L1: np.zeros((7, 3))})
    with pytest.raises(ValueError, match="no points"):
        s.posterior_summary({X0: np.zeros((0, 3)), L1: np.zeros((0, 2))})
    for w, match in ((np.ones(6), r"\[n\] = \[7\]"), (np.ones((7, 1)), r"\[n\]"), (-np.ones(7), "non-negative"),
                     (np.zeros(7), "all zero"), (np.array([1, 1, np.nan, 1, 1, 1, 1.0]), "finite"),
                     (np.array([1, 1, np.inf, 1, 1, 1, 1.0]), "finite")):
        with pytest.raises(ValueError, match=match):
            s.posterior_summary(own, weights=w)
    for q in ([0.5, 1.01], [-0.1], [float("nan")], []):
        with pytest.raises(ValueError, match="probabilities"):
            s.posterior_summary(own, quantiles=q)
    with pytest.raises(ValueError, match="unweighted"):
        s.posterior_summary(own, quantiles=[0.5], weights=np.ones(7))
    with pytest.raises(ValueError, match="at most 16384 points"):
        s.posterior_summary({X0: np.zeros((16385, 3)), L1: np.zeros((16385, 2))}, quantiles=[0.5])
    with pytest.raises(ValueError, match=r"truth of X0 must be \[3\]"):
        s.posterior_summary(own, truth={X0: np.zeros(2)})
    with pytest.raises(ValueError, match="truth holds none"):
        s.posterior_summary(own, truth={X9: np.zeros(3)})
    # a pair wider than 16 columns: two 9-column variables put into the ordering by hand
    W1, W2 = Variable("W1", 9), Variable("W2", 9)
    s._elimination_ordering = list(s._elimination_ordering) + [W1, W2]
    with pytest.raises(ValueError, match="18 columns wide"):
        s.posterior_summary({**own, W1: np.zeros((7, 9)), W2: np.zeros((7, 9))}, pairs=[(W1, W2)])
    assert refuse.calls == 0


# ---- the host functions against the reference's own values ------------------------------------------------------------------
def fixture_case(fx, k):
    """(variables, float32 samples, reference means, {variable: its reference mean}, {variable: the other assignment})."""
    kinds = [str(s) for s in fx["kinds%d" % k]]
    variables = [SE2Variable("X%d" % i) if kind == "SE2" else R2Variable("L%d" % i, VariableType.Landmark)
                 for i, kind in enumerate(kinds)]
    means, other = fx["means%d" % k], fx["other%d" % k]
    var2mean, var2other, at = {}, {}, 0
    for v in variables:
        var2mean[v], var2other[v] = means[at:at + v.dim], other[at:at + v.dim]
        at += v.dim
    return variables, fx["samples%d" % k], means, var2mean, var2other


def test_host_functions_equal_the_reference_values():
    fx = np.load(os.path.join(GOLDEN, "sample_summary.npz"))
    assert int(fx["n_cases"]) == 4
    straddles = False
    for k in range(int(fx["n_cases"])):
        variables, x, means, var2mean, var2other = fixture_case(fx, k)
        assert x.dtype == np.float32 and x.shape[1] == sum(v.dim for v in variables) == means.size
        for got, key in ((ST.translation_distance(var2mean, var2other), "translation"),
                         (ST.geodesic_distance(var2mean, var2other), "geodesic"),
                         (ST.rmse(x.astype(np.float64), fx["rmse_other%d" % k]), "rmse")):
            want = float(fx["%s%d" % (key, k)])
            print(k, key, got, want)
            assert abs(got - want) <= 1e-12 * abs(want), (k, key, got, want)
        terms = ST.translation_terms(var2mean, var2other)
        assert list(terms) == variables
        assert abs(np.sqrt(sum(terms.values()) / len(variables)) - float(fx["translation%d" % k])) <= 1e-12
        at = 0
        for v in variables:
            if v.dim == 3:
                th = x[:, at + 2]
                straddles |= bool(th.max() > 3.0 and th.min() < -3.0)
            at += v.dim
    assert straddles                                              # one heading has mass on both sides of +-pi
    with pytest.raises(ValueError, match="shape"):
        ST.rmse(np.zeros((3, 2)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match="Unknown variable type"):
        ST.translation_distance({Variable("W", 4): np.zeros(4)}, {Variable("W", 4): np.zeros(4)})
    with pytest.raises(ValueError, match="Unknown variable type"):
        ST.geodesic_distance({Variable("W", 4): np.zeros(4)}, {Variable("W", 4): np.zeros(4)})


def test_the_oracle_itself():
    """`oracle_moments` against numpy on a benign column, the circular mean against scipy, `oracle_quantiles` at the ends."""
    from scipy.stats import circmean
    rng = np.random.RandomState(3)
    x = np.stack([rng.standard_normal(50) * 2 + 5, wrap_pi(rng.standard_normal(50) * 0.3 + 3.1), np.full(50, 7.25)], axis=1)
    x = x.astype(np.float32)
    mean, res, cov, s = oracle_moments(x, [0, 1, 2], [0, 1, 0])
    x64 = x.astype(np.float64)
    assert abs(mean[0] - x64[:, 0].mean()) <= 1e-14 and mean[2] == 7.25 and cov[2, 2] == 0.0 and s[2] == 0.0
    assert abs(wrap_pi(mean[1] - circmean(x64[:, 1], high=np.pi, low=-np.pi))) <= 1e-14
    assert abs(cov[0, 0] - x64[:, 0].var()) <= 1e-14 and np.isnan(res[0]) and 0.9 < res[1] <= 1.0
    w = rng.uniform(size=50)
    w[::10] = 0.0
    mean_w, _, cov_w, _ = oracle_moments(x, [0, 2], None, w)
    assert abs(mean_w[0] - np.average(x64[:, 0], weights=w)) <= 1e-14 and mean_w[1] == 7.25 and cov_w[1, 1] == 0.0
    q, srt = oracle_quantiles(x, 0, [0.0, 0.5, 1.0])
    assert q[0] == srt[0] and q[2] == srt[-1] and q[1] == np.median(x64[:, 0])
