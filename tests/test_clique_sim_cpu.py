"""The fused clique simulator (csrc/clique_sim.hip) pinned sample by sample -- the half that needs no GPU.

`oracle/clique_sim_ref.py` replays the kernel's contract in numpy: Philox4x32-10 and the float32 uniforms bit for bit, the
rest in float64.  Here:

  * the generator against the published known answers of Philox4x32-10 (the Random123 vectors), and the range of the
    uniforms, (0, 1] with 1.0 reached;
  * the replay standing in for the launch under `FusedSimulationBackend`: it draws the host simulator's distribution
    (the bounds of tests/test_surface_gpu.py::test_device_batch_simulator_matches_host_simulator_in_distribution), which
    ties the replay's reading of the contract to the factors' own samplers independently of the device;
  * the 150-column cap: `run_plan` declines, the solver simulates that clique on the host, nothing is launched;
  * the schedules of tests/test_clique_sim_gpu.py (they are built here and imported there) with their tolerance.

Tolerance of the per-sample comparison.  For a schedule, E_c = the largest difference in column c between the float64
replay and the SAME formulas evaluated with every intermediate in numpy float32 -- the reference against itself, never the
kernel.  The device must satisfy |dev - f64| <= 4 E_c + 2^-23 max|column c| (angles modulo 2 pi): the factor 4 covers
ocml's sinf / cosf / logf / fmodf within a few ulp, FMA contraction and one more rounding in two_pi * u.  Measured E_c
(largest over the columns of that kind; n = 600 unless stated), and next to it, as information only, the largest
|dev - f64| / tolerance an MI355X showed:

  schedule                                E_c translations   E_c headings    device / tolerance
  raw draws, four seeds                   9.9e-6 (10 z0)     9.6e-7          0.27
  every op, inputs to +-50 m              1.8e-5             1.6e-6          0.31
  small heading noise, l22 1e-2 .. 0      2.8e-6             8.6e-7          0.27
  scratch columns, n = 1 .. 600           2.5e-6             3.2e-7          0.23
  wide launches, D_total 48 .. 150        1.3e-5             7.6e-7          0.25
  40 ops                                  3.8e-6             -               0.29
  the eight-factor clique, n = 1000       4.5e-6             3.5e-7          0.26

(The raw draws' largest E_c is the column 10 z0: float32(2 pi) is 1.7e-7 off 2 pi, and two_pi * u rounds once more; both
the float32 replay and the kernel carry that, the float64 replay does not.)

With the float32-cancelling (1 - cos w) / w that `se2_exp` used before, the float32 replay itself misses this bound on
the small-heading-noise schedules by a factor of 45 to 64 (test_cancelling_exp_map_misses_the_bound), so does any kernel
that evaluates it.
"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import clique_sim_ref as R

SEEDS = (0, 2 ** 32 + 5, 2 ** 62 - 1, 2 ** 64 - 1)
COV3 = np.array([[0.09, 0.02, -0.004], [0.02, 0.04, 0.006], [-0.004, 0.006, 0.0025]])
_L3 = np.linalg.cholesky(COV3)
LP6 = [_L3[0, 0], _L3[1, 0], _L3[1, 1], _L3[2, 0], _L3[2, 1], _L3[2, 2]]          # a full Cholesky factor, SE(2)
_L2 = np.linalg.cholesky(np.array([[0.5, 0.2], [0.2, 0.3]]))
LP3 = [_L2[0, 0], _L2[1, 0], _L2[1, 1]]                                              # ... and R2
MIX_W = 0.7


def rec(code, a=0, b=0, c=0, k=0, p=(), cand=(), src=0):
    """A plain record with the fields of `nfisam_sim_op`; `src` of a COPY is a key into the case's sources."""
    p = [float(np.float32(v)) for v in p] + [0.0] * (9 - len(p))
    return types.SimpleNamespace(code=code, a=a, b=b, c=c, k=k, p=p, cand=list(cand) + [0] * (4 - len(cand)), src=src)


def case(name, ops, n, D_out, D_total, seed, sources=None, angles=()):
    return dict(name=name, ops=ops, n=n, D_out=D_out, D_total=D_total, seed=seed, sources=sources or {},
                angles=[c for c in angles if c < D_out])


def poses(rng, n, reach):
    return np.column_stack([rng.uniform(-reach, reach, (n, 2)), rng.uniform(-np.pi, np.pi, n)]).astype(np.float32)


# ---- the schedules -------------------------------------------------------------------------------------------------------
def raw_draws_case(seed, n=600):
    """Ops that expose the generator's outputs directly.  Columns: 0-1, 2-3 the same copied point | 4-5 (z0, z1) |
    6-8 (0, 0, wrap z2) | 9-10 (cos phi, sin phi), phi = (2 u2 - 1) pi | 11 sigma(u2 < w) z0 | 12-13 point + sigma(u3 < w) z0 (cos, sin)"""
    pt = np.tile(np.array([[0.5, -0.25]], dtype=np.float32), (n, 1))
    ops = [rec(R.COPY, a=2, b=0, c=0, k=2, src=1), rec(R.COPY, a=2, b=0, c=2, k=2, src=1),
           rec(R.PRIOR_R2, c=4, p=[0, 0, 1, 0, 1]), rec(R.PRIOR_SE2, c=6, p=[0, 0, 0, 0, 0, 0, 0, 0, 1]),
           rec(R.PRIOR_R2_RING, c=9, p=[0, 0, 1, 0]), rec(R.NH_OBS, a=0, b=2, c=11, p=[1, 10, MIX_W]),
           rec(R.NH_RING, a=0, c=12, p=[0, 1, 10, MIX_W])]
    return case("raw draws, seed %d" % seed, ops, n, 14, 14, seed, {1: pt}, angles=[8])


def all_ops_case(n=600):
    """All 15 codes with noise.  Columns: 0-2 A, 3-5 B (poses), 6-7 P, 8-9 Q, 10-11 R (points), then one op after the other."""
    rng = np.random.RandomState(11)
    src = np.column_stack([poses(rng, n, 50.0), poses(rng, n, 50.0), rng.uniform(-50, 50, (n, 6))]).astype(np.float32)
    ops = [rec(R.COPY, a=12, b=0, c=0, k=12, src=1),
           rec(R.PRIOR_SE2, c=12, p=[20.0, -30.0, 2.5] + LP6),
           rec(R.REL_FWD, a=0, c=15, p=[5.0, 0.5, 0.4] + LP6), rec(R.REL_FWD, a=15, c=18, p=[5.0, -0.5, -0.2] + LP6),
           rec(R.REL_FWD, a=18, c=21, p=[4.0, 0.7, 1.1] + LP6), rec(R.REL_BWD, a=21, c=24, p=[2.0, -0.5, -2.9] + LP6),
           rec(R.REL_OBS, a=0, b=24, c=27, p=[0, 0, 0] + LP6),
           rec(R.RING, a=0, c=30, p=[12.0, 0.5]), rec(R.RANGE_OBS, a=12, b=30, c=32, p=[0.5]),
           rec(R.ADA_OBS, a=21, c=33, k=3, cand=[6, 8, 10], p=[0.2, 0.7, 1.0, 1.0, 0.5]),
           rec(R.ADA_OBS, a=24, c=34, k=4, cand=[6, 8, 10, 30], p=[0.1, 0.5, 0.8, 1.0, 0.5]),
           rec(R.NH_RING, a=3, c=35, p=[9.0, 0.5, 3.0, MIX_W]), rec(R.NH_OBS, a=3, b=35, c=37, p=[0.5, 3.0, MIX_W]),
           rec(R.PRIOR_R2, c=38, p=[5.0, -3.0] + LP3), rec(R.PRIOR_R2_RING, c=40, p=[1.0, 2.0, 7.0, 0.5]),
           rec(R.REL_R2_FWD, a=6, c=42, p=[5.0, -5.0] + LP3), rec(R.REL_R2_BWD, a=8, c=44, p=[5.0, -5.0] + LP3),
           rec(R.REL_R2_OBS, a=42, b=44, c=46, p=[0, 0] + LP3)]
    assert sorted(set(o.code for o in ops)) == list(range(1, 16))
    return case("every op", ops, n, 48, 48, 2 ** 40 + 977, {1: src}, angles=[2, 5, 14, 17, 20, 23, 26, 29])


HEADING_NOISE = (1e-2, 1e-3, 1e-4, 1e-6, 0.0)


def small_heading_case(l22, n=600):
    """Translation noise 1 m, heading noise l22: |w| covers 1e-8 .. 1e-2 over the five values, and both sides of the
    series branch of the exponential map.  Columns: 0-2 A, 3-5 B | prior | A * rel | B * rel^-1 | (A^-1 B) * Exp."""
    rng = np.random.RandomState(5)
    src = np.column_stack([poses(rng, n, 5.0), poses(rng, n, 5.0)])
    L = [1.0, 0.0, 1.0, 0.0, 0.0, l22]
    ops = [rec(R.COPY, a=6, b=0, c=0, k=6, src=1), rec(R.PRIOR_SE2, c=6, p=[1.0, -2.0, 0.3] + L),
           rec(R.REL_FWD, a=0, c=9, p=[2.0, 0.5, 0.4] + L), rec(R.REL_BWD, a=3, c=12, p=[2.0, -0.5, -0.2] + L),
           rec(R.REL_OBS, a=0, b=3, c=15, p=[0, 0, 0] + L)]
    return case("small heading noise %g" % l22, ops, n, 18, 18, 2 ** 33 + 17, {1: src}, angles=[2, 5, 8, 11, 14, 17])


SHAPE_N = (1, 255, 256, 257, 600)


def scratch_case(n):
    """D_out < D_total: a pose drawn into scratch columns 5-7 and used from the output columns 0-2 (odometry) and 3-4 (ring)."""
    ops = [rec(R.PRIOR_SE2, c=5, p=[1.0, -2.0, 0.3] + LP6), rec(R.REL_FWD, a=5, c=0, p=[5.0, 0.5, 0.4] + LP6),
           rec(R.RING, a=5, c=3, p=[12.0, 0.5])]
    cs = case("scratch columns, n = %d" % n, ops, n, 5, 8, 2 ** 62 - 1, angles=[2])
    # The five sizes are one test with one set of inputs: sample q is the same draw at every n, so the rows of a smaller
    # run are the first rows of the largest one.  E_c is measured over all of them, i.e. on the largest (the E_c of a run
    # of one sample would be a lottery ticket: 6e-9 rad here, a tenth of an ulp).
    cs["bound_from"] = None if n == SHAPE_N[-1] else (scratch_case, SHAPE_N[-1])
    return cs


WIDE_D = (48, 49, 64, 65, 150)


def wide_case(D_total, n=600):
    """One wide COPY (k = D_total - 10) and random ops in the top ten columns, two of which read the COPY's last columns."""
    k = D_total - 10
    src = np.random.RandomState(D_total).uniform(-50, 50, (n, k)).astype(np.float32)
    ops = [rec(R.COPY, a=k, b=0, c=0, k=k, src=1), rec(R.PRIOR_SE2, c=k, p=[20.0, -30.0, 2.5] + LP6),
           rec(R.REL_FWD, a=k, c=k + 3, p=[5.0, 0.5, 0.4] + LP6), rec(R.RING, a=k - 2, c=k + 6, p=[12.0, 0.5]),
           rec(R.RANGE_OBS, a=k - 2, b=k + 6, c=k + 8, p=[0.5]), rec(R.NH_OBS, a=k, b=k + 6, c=k + 9, p=[0.5, 3.0, MIX_W])]
    return case("wide launch, D_total = %d" % D_total, ops, n, D_total, D_total, 2 ** 32 + 5, {1: src},
                angles=[k + 2, k + 5])


def forty_ops_case(n=257):
    ops = [rec(R.PRIOR_R2, c=2 * o, p=[o, -o] + LP3) for o in range(R.MAX_OPS)]
    return case("40 ops", ops, n, 80, 80, 31337)


def eight_factor_set():
    """The clique of test_device_batch_simulator_matches_host_simulator_in_distribution: an SE(2) prior, two odometry
    steps, ranges to two landmarks, a 2-way ambiguous association and a possibly-outlier range -> (factors, pattern)."""
    from factors.Factors import (AmbiguousDataAssociationFactor, BinaryFactorWithNullHypo,
                                 SE2R2RangeGaussianLikelihoodFactor, SE2RelativeGaussianLikelihoodFactor,
                                 UnarySE2ApproximateGaussianPriorFactor)
    from slam.Variables import R2Variable, SE2Variable, VariableType
    X = [SE2Variable("X%d" % i) for i in range(3)]
    L0, L1 = R2Variable("L0", VariableType.Landmark), R2Variable("L1", VariableType.Landmark)
    odom_cov = np.diag([0.2, 0.04, 0.02]) ** 2
    fs = [UnarySE2ApproximateGaussianPriorFactor(X[0], np.array([1.0, -2.0, 0.3]), np.diag([0.3, 0.2, 0.05]) ** 2),
          SE2RelativeGaussianLikelihoodFactor(X[0], X[1], np.array([5.0, 0.5, 0.4]), odom_cov),
          SE2RelativeGaussianLikelihoodFactor(X[1], X[2], np.array([5.0, -0.5, -0.2]), odom_cov),
          SE2R2RangeGaussianLikelihoodFactor(X[0], L0, 12.0, 0.5),
          SE2R2RangeGaussianLikelihoodFactor(X[1], L1, 9.0, 0.5),
          SE2R2RangeGaussianLikelihoodFactor(X[2], L0, 11.0, 0.5),
          AmbiguousDataAssociationFactor(X[2], [L0, L1], np.array([0.5, 0.5]), SE2R2RangeGaussianLikelihoodFactor, 10.0,
                                         0.5),
          BinaryFactorWithNullHypo(X[1], L0, np.array([0.7, 0.3]), SE2R2RangeGaussianLikelihoodFactor, 11.5, 0.5,
                                   null_sigma_scale=6.0)]
    return fs, [L0, L1] + X


# ---- reference and tolerance ---------------------------------------------------------------------------------------------
def col_diff(x, y, angles):
    """|x - y| column by column, angle columns modulo 2 pi."""
    d = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64))
    for c in angles:
        d[:, c] = np.abs((d[:, c] + np.pi) % (2 * np.pi) - np.pi)
    return d


def reference(cs):
    """-> (float64 replay [n, D_out], tolerance [D_out], E [D_out]) of a case (see the module's docstring)."""
    args = (cs["ops"], cs["n"], cs["D_out"], cs["D_total"], cs["seed"], cs["sources"])
    r64 = R.replay(*args, dtype=np.float64)
    r32 = R.replay(*args, dtype=np.float32)
    assert r64.dtype == np.float64 and r32.dtype == np.float32 and r64.shape == r32.shape == (cs["n"], cs["D_out"])
    E = col_diff(r32, r64, cs["angles"]).max(0)
    return r64, 4.0 * E + 2.0 ** -23 * np.abs(r64).max(0), E


@functools.lru_cache(maxsize=None)
def cached(builder, *args):
    """A case and its reference, computed once per session and shared (read-only) among the tests."""
    cs = builder(*args)
    ref = reference(cs)
    if cs.get("bound_from"):
        whole = cached(*cs["bound_from"])[1]
        assert np.array_equal(ref[0], whole[0][:cs["n"]])
        ref = (ref[0], whole[1], whole[2])
    for a in ref:
        a.setflags(write=False)
    return cs, ref


def mmd_rbf(a, b, sigma):
    def k(x, y):
        d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
        return np.exp(-d / (2 * sigma ** 2))
    return float(np.sqrt(max(k(a, a).mean() + k(b, b).mean() - 2 * k(a, b).mean(), 0)))


# ---- tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox4x32_10_known_answers(counter, key, out):
    """The Random123 known-answer vectors of Philox4x32-10."""
    words = R.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(w[0]) for w in words) == out
    # vectorised over the first counter word: same words
    many = R.philox4x32_10((np.array([counter[0], 7], dtype=np.uint64),) + tuple(counter[1:]), key)
    assert " ".join("%08x" % int(w[0]) for w in many) == out and all(w.shape == (2,) for w in many)


def test_uniforms_lie_in_0_1_with_1_reached():
    """u = (float32(c >> 8) + 0.5f) * 2^-24: x + 0.5 is not representable for x >= 2^23 and rounds to even, so the largest
    value is exactly 1.0 and the smallest 2^-25 -- the draw is on (0, 1]; log u <= 0 and the bearing (2u - 1) pi <= pi."""
    u = R.unit_float32(np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xfffffeff, 0xffffff00, 0xffffffff], dtype=np.uint64))
    assert u.dtype == np.float32
    np.testing.assert_array_equal(u, np.array([2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, (2 ** 23 - 0.5) * 2.0 ** -24, 0.5,
                                               1.0 - 2.0 ** -23, 1.0, 1.0], dtype=np.float32))
    # the key's upper word matters: seeds that agree in their low 32 bits give different draws
    a, b = R.uniforms(5, 64, 3), R.uniforms(2 ** 32 + 5, 64, 3)
    assert all(0 < x.min() and x.max() <= 1 for x in a + b) and not np.any(a[0] == b[0])
    # (sample, op) is the counter: a stream of its own per op index and per sample
    c = R.uniforms(5, 64, 4)
    assert not np.any(a[0] == c[0]) and len(np.unique(a[0])) == 64


def test_replay_as_the_launch_draws_the_host_simulators_distribution(monkeypatch):
    """`FusedSimulationBackend` with the replay in place of the kernel launch against the factors' numpy samplers:
    the per-column moment bounds and the MMD-against-floor bound of the GPU test of the same clique."""
    import nfisam_hip as nh
    from sampler.DeviceSimulation import FusedSimulationBackend
    from sampler.SimulationBasedSampler import SimulationBasedSampler
    calls = []

    def replay_launch(ops, n, D_out, D_total, seed, device):
        calls.append((len(ops), D_out, D_total))
        return torch.from_numpy(R.replay(ops, n, D_out, D_total, seed, {}).astype(np.float32))
    monkeypatch.setattr(nh, "simulate_clique", replay_launch)
    fs, order = eight_factor_set()
    n = 6000
    np.random.seed(0); torch.manual_seed(0)
    host, hv, hobs = SimulationBasedSampler(fs, order).sample(n)
    dev_s, dv, dobs = SimulationBasedSampler(fs, order).sample(n, backend=FusedSimulationBackend("cpu"))
    assert calls == [(8, host.shape[1], host.shape[1])]
    assert dev_s.dtype == torch.float32 and tuple(dev_s.shape) == host.shape
    assert [str(v.name) for v in hv] == [str(v.name) for v in dv]
    np.testing.assert_array_equal(hobs, dobs)
    d = dev_s.numpy().astype(np.float64)
    for c in range(host.shape[1]):
        sd = host[:, c].std()
        assert abs(host[:, c].mean() - d[:, c].mean()) < 0.08 * sd + 5e-3, (c, host[:, c].mean(), d[:, c].mean())
        assert abs(d[:, c].std() / sd - 1.0) < 0.06, (c, sd, d[:, c].std())
    perm = np.random.RandomState(1).permutation(n)
    host, d = host[perm], d[perm]
    scale = host.std(0)
    a, b = host[:1500] / scale, d[:1500] / scale
    floor = mmd_rbf(host[:1500] / scale, host[1500:3000] / scale, np.sqrt(host.shape[1]))
    assert mmd_rbf(a, b, np.sqrt(host.shape[1])) < max(0.03, 3 * floor)


def test_column_cap_makes_the_backend_decline_and_the_solver_simulate_on_the_host(monkeypatch):
    """A column plan beyond the kernel's 150 columns: `run_plan` raises `DeviceSimulationUnsupported` (in the batch
    itself, or only with the scratch columns), `clique_training_sampler` returns the host batch, nothing is launched."""
    import nfisam_hip as nh
    import sampler.DeviceSimulation as DS
    from factors.Factors import UnarySE2ApproximateGaussianPriorFactor
    from sampler.SimulationBasedSampler import SimulationBasedSampler
    from slam.FactorGraphSolver import FactorGraphSolver
    from slam.Variables import Variable
    launches, messages = [], []
    monkeypatch.setattr(nh, "simulate_clique", lambda *a, **k: launches.append(a) or torch.zeros(a[1], a[2]))
    assert DS.MAX_COLUMNS * 256 * 4 == 150 * 1024

    class Message(UnarySE2ApproximateGaussianPriorFactor.__mro__[1]):          # ExplicitPriorFactor: a child's flow, stubbed
        def __init__(self, vs):
            self._vs = vs

        @property
        def vars(self):
            return self._vs

        def sample(self, n, **kw):
            return np.random.randn(n, sum(v.dim for v in self._vs))

        def sample_on_device(self, n):
            messages.append(n)
            return torch.zeros(n, sum(v.dim for v in self._vs))

    class Solver(FactorGraphSolver):
        def __init__(self, factors, pattern):
            self._working_graph = types.SimpleNamespace(get_clique_factor_graph=lambda c: types.SimpleNamespace(factors=factors))
            self._working_bayes_tree = types.SimpleNamespace(clique_variable_pattern=lambda c: pattern)

        def _simulation_backend(self):
            return DS.FusedSimulationBackend("cpu")
    vs = [Variable("V%d" % i, 8) for i in range(19)]                            # 152 columns in 19 COPY ops
    # (a) the batch alone is too wide: declined before a child's message is sampled
    with pytest.raises(DS.DeviceSimulationUnsupported, match="152 columns"):
        SimulationBasedSampler([Message(vs)], vs).sample(10, backend=DS.FusedSimulationBackend("cpu"))
    assert messages == [] and launches == []
    # (b) 144 batch columns + one scratch variable
    with pytest.raises(DS.DeviceSimulationUnsupported, match="152 columns"):
        SimulationBasedSampler([Message(vs)], vs[:18]).sample(10, backend=DS.FusedSimulationBackend("cpu"))
    assert messages == [10] and launches == []
    for pattern in (vs, vs[:18]):
        batch, order, obs = Solver([Message(vs)], pattern).clique_training_sampler(None, 10, "direct")
        assert isinstance(batch, np.ndarray) and batch.shape == (10, 8 * len(pattern)) and order == pattern and len(obs) == 0
    assert launches == []
    # exactly at the cap the backend launches
    x, order, _ = Solver([Message(vs[:18]), Message([Variable("W", 6)])], vs[:18]).clique_training_sampler(None, 10, "direct")
    assert isinstance(x, torch.Tensor) and len(launches) == 1 and launches[0][1:4] == (10, 144, 150)


ALL_CASES = [(raw_draws_case, s) for s in SEEDS] + [(all_ops_case,)] + [(small_heading_case, l) for l in HEADING_NOISE] + \
    [(scratch_case, n) for n in SHAPE_N[::-1]] + [(wide_case, D) for D in WIDE_D] + [(forty_ops_case,)]


@pytest.mark.parametrize("which", ALL_CASES, ids=lambda w: "-".join([w[0].__name__] + [str(a) for a in w[1:]]))
def test_tolerance_is_float32_rounding_of_the_schedule(which):
    """The tolerance the device is held to comes from the reference alone and is tight: a few float32 roundings of the
    column's magnitude (2^-23 |x| is one ulp), never more than 1e-4 m / 1e-5 rad at coordinates of +-50 m -- a hundredth of
    the 1e-4 m error of a cancelling exponential map at 1 m of noise is visible at small coordinates."""
    cs, (r64, tol, E) = cached(*which)
    assert np.all(np.isfinite(r64)) and np.all(E <= 64 * 2.0 ** -24 * np.maximum(np.abs(r64).max(0), 1.0))
    assert tol.max() < 1e-4 and all(tol[c] < 1e-5 for c in cs["angles"])
    print("%-32s E_c: translations %.2e  headings %.2e" % (
        cs["name"], max([E[c] for c in range(cs["D_out"]) if c not in cs["angles"]]),
        max([E[c] for c in cs["angles"]] or [0.0])))


@pytest.mark.parametrize("l22", HEADING_NOISE[:3])
def test_cancelling_exp_map_misses_the_bound(l22):
    """b = (1 - cos w) / w in float32 is 0 up to |w| ~ 2.4e-4 and noisy beyond: the float32 replay with that form -- what
    the kernel computed before -- misses the tolerance of the small-heading-noise schedules; with the stable form it is
    inside by construction (4x)."""
    cs, (r64, tol, E) = cached(small_heading_case, l22)
    args = (cs["ops"], cs["n"], cs["D_out"], cs["D_total"], cs["seed"], cs["sources"])
    old = col_diff(R.replay(*args, dtype=np.float32, _cancelling_exp=True), r64, cs["angles"])
    new = col_diff(R.replay(*args, dtype=np.float32), r64, cs["angles"])
    assert np.all(new <= tol)
    xy = [c for c in range(6, 18) if c not in cs["angles"]]
    worst = (old / tol).max(0)
    print("l22 = %g: cancelling form reaches %.1f x the tolerance" % (l22, worst[xy].max()))
    assert all(worst[c] > 3.0 for c in xy), worst
