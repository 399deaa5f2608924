"""The Metropolis kernels on the GPU (nfisam_sample_propose, nfisam_sample_accept, nfisam_hip.sample_propose_t /
sample_accept_t, utils.Statistics.metropolis_refine_t, NFiSAM.posterior_mcmc) against the float64 numpy restatement of
tests/test_sample_mcmc_cpu.py: n in {1, 2, 63, 64, 65, 130} x rows in {1, 3, 4, 5, 67, slab - 1, slab, slab + 1}, wrapped rows
with a pair across the +-pi seam, frozen rows, with and without the scores.

Bounds, none of them measured:
  * a proposal: within one float32 ulp of the restatement's (the normals differ by ulps of float64: a value may round the other
    way), through the wrapped difference on an angle's row; a frozen row is Xt's bits;
  * log alpha, fed the device's own proposals: within B = 4 (rows + 16) 2^-53 (sum |terms| + |lp_x| + |lp_y|), the summation
    bound of the CPU file; the decisions are then IDENTICAL, because no chain of the fixture lies within B of its decision;
  * everything else is bit for bit."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_mcmc_cpu import (KAPPA, MU, SIGMA, T_H, T_N, T_SEED, T_START, T_STEPS, T_WRAP, THETA0, accept, assert_decidable,
                                  assert_target_conditions, decision_case, decision_cases, propose, rounding_bound, signed_wrap)
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PI = np.pi


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def dev_propose(c, cols=None):
    sl = slice(None) if cols is None else slice(0, cols)
    Xt = _t(c["Xt"][:, sl])
    keep = Xt.clone()
    Yt = nh.sample_propose_t(Xt, _t(None if c["Gx"] is None else c["Gx"][:, sl]), c["h"], c["wrap"], c["seed"], c["t"])
    assert np.array_equal(_bits(keep), _bits(Xt))                      # Xt is untouched
    return Yt


def dev_accept(c, Yt, cols=None, lp_x=None, lp_y=None, Gy=None):
    sl = slice(None) if cols is None else slice(0, cols)
    drift = c["Gx"] is not None
    Xt, Gx = _t(c["Xt"][:, sl]), _t(c["Gx"][:, sl]) if drift else None
    Gy = _t((c["Gy"] if Gy is None else Gy)[:, sl]) if drift else None
    lx, ly = _t((c["lp_x"] if lp_x is None else lp_x)[sl]), _t((c["lp_y"] if lp_y is None else lp_y)[sl])
    keep = (Yt.clone(), None if Gy is None else Gy.clone(), ly.clone())
    la, acc = nh.sample_accept_t(Xt, Yt, Gx, Gy, lx, ly, c["h"], c["wrap"], c["seed"], c["t"])
    assert np.array_equal(_bits(keep[0]), _bits(Yt)) and np.array_equal(_bits(keep[2]), _bits(ly))
    assert Gy is None or np.array_equal(_bits(keep[1]), _bits(Gy))
    return dict(log_alpha=la.cpu().numpy(), accepted=acc.cpu().numpy(), X=Xt.cpu().numpy(),
                G=None if Gx is None else Gx.cpu().numpy(), lp=lx.cpu().numpy())


def assert_same_state(got, want):
    """The state after a step, bit for bit: accepted columns are the proposal's bits, rejected ones untouched."""
    assert np.array_equal(got["accepted"], want["accepted"])
    assert np.array_equal(_bits(got["X"]), _bits(want["X"].astype(np.float32)))
    assert np.array_equal(_bits(got["lp"]), _bits(want["lp"]))
    if want["G"] is not None:
        assert np.array_equal(_bits(got["G"]), _bits(np.ascontiguousarray(want["G"])))


# ---- 1. the proposal against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [True, False])
def test_propose_matches_the_restatement(drift):
    worst = 0.0
    for c in decision_cases(drift):
        Yd = dev_propose(c).cpu().numpy()
        Yr = propose(c["Xt"], c["Gx"], c["h"], c["wrap"], c["seed"], c["t"])
        x_rows = c["Xt"].shape[0]
        wrap = np.zeros(x_rows, dtype=bool) if c["wrap"] is None else c["wrap"].astype(bool)
        frozen = c["h"] == 0
        assert np.array_equal(_bits(Yd[frozen]), _bits(c["Xt"][frozen]))
        assert np.all(np.isfinite(Yd))
        diff = Yd.astype(np.float64) - Yr.astype(np.float64)
        diff[wrap] = signed_wrap(diff[wrap])
        ulp = np.spacing(np.maximum(np.abs(Yd), np.abs(Yr)).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(diff) <= ulp), (c["Xt"].shape, float(np.max(np.abs(diff) / ulp)))
        worst = max(worst, float(np.max(np.abs(diff) / ulp)))
        assert np.all((Yd[wrap & ~frozen] >= -np.float32(PI)) & (Yd[wrap & ~frozen] < np.float32(PI)))
    print("drift = %s: the largest |device - restatement| of a proposal = %.2f float32 ulp" % (drift, worst))


# ---- 2. the accept step, fed the device's own proposals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [True, False])
def test_accept_matches_the_restatement(drift):
    worst, count = 0.0, np.zeros(2, dtype=np.int64)
    for c in decision_cases(drift):
        Yt = dev_propose(c)
        ref = accept(c["Xt"], Yt.cpu().numpy(), c["Gx"], c["Gy"], c["lp_x"], c["lp_y"], c["h"], c["wrap"], c["seed"], c["t"])
        assert_decidable(c, ref)                                       # (the fixture's property holds for the device's Yt too)
        got = dev_accept(c, Yt)
        B = rounding_bound(c["Xt"].shape[0], ref["abs_sum"])
        err = np.abs(got["log_alpha"] - ref["log_alpha"])
        assert np.all(err <= B), (c["Xt"].shape, float(np.max(err / B)))
        worst = max(worst, float(np.max(err / B)))
        assert_same_state(got, ref)
        count += np.bincount(ref["accepted"], minlength=2)
    print("drift = %s: the largest |log alpha - restatement| / B = %.3g; %d accepted, %d rejected" % (drift, worst, count[1], count[0]))


def test_accept_special_values():
    """lp_y = -inf rejects, lp_x = -inf with a finite lp_y accepts, a NaN log alpha rejects -- whatever its source."""
    c = decision_case(5, 65, True)
    Yt = dev_propose(c)
    lp_x, lp_y, Gy = c["lp_x"].copy(), c["lp_y"].copy(), c["Gy"].copy()
    lp_y[0], lp_x[1], lp_y[2], lp_x[3], lp_y[3], lp_x[5] = -np.inf, -np.inf, np.nan, -np.inf, -np.inf, np.nan
    Gy[0, 4] = np.nan
    ref = accept(c["Xt"], Yt.cpu().numpy(), c["Gx"], Gy, lp_x, lp_y, c["h"], c["wrap"], c["seed"], c["t"])
    got = dev_accept(c, Yt, lp_x=lp_x, lp_y=lp_y, Gy=Gy)
    assert list(got["accepted"][:6]) == [0, 1, 0, 0, 0, 0]
    assert got["log_alpha"][1] == np.inf and got["log_alpha"][0] == -np.inf and np.all(np.isnan(got["log_alpha"][[2, 3, 4, 5]]))
    assert_same_state(got, ref)
    # the same rules without the scores (the symmetric form)
    s = decision_case(5, 65, False)
    Ys = dev_propose(s)
    ref = accept(s["Xt"], Ys.cpu().numpy(), None, None, lp_x, lp_y, s["h"], s["wrap"], s["seed"], s["t"])
    got = dev_accept(s, Ys, lp_x=lp_x, lp_y=lp_y)
    assert list(got["accepted"][:4]) == [0, 1, 0, 0] and got["accepted"][5] == 0
    assert_same_state(got, ref)


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [True, False])
def test_bits(drift):
    c = decision_case(67, 130, drift)
    Y = dev_propose(c)
    assert np.array_equal(_bits(Y), _bits(dev_propose(c)))
    assert not np.array_equal(_bits(Y), _bits(dev_propose(dict(c, t=c["t"] + 1))))
    assert not np.array_equal(_bits(Y), _bits(dev_propose(dict(c, seed=c["seed"] ^ 1))))
    a, b = dev_accept(c, Y), dev_accept(c, Y)
    assert np.array_equal(_bits(a["log_alpha"]), _bits(b["log_alpha"]))
    assert_same_state(a, b)
    # the uniform alone depends on t and the seed: with every log alpha near -0.7 a chain accepts with probability 1 / 2
    even = c["lp_y"] - a["log_alpha"] - 0.7
    e0, e1, e2 = (dev_accept(k, Y, lp_y=even) for k in (c, dict(c, t=c["t"] + 1), dict(c, seed=c["seed"] ^ 1)))
    assert np.array_equal(_bits(e0["log_alpha"]), _bits(e1["log_alpha"])) and np.array_equal(_bits(e0["log_alpha"]), _bits(e2["log_alpha"]))
    assert np.all(np.abs(e0["log_alpha"] + 0.7) < 1e-9) and 30 < int(e0["accepted"].sum()) < 100
    assert not np.array_equal(e0["accepted"], e1["accepted"]) and not np.array_equal(e0["accepted"], e2["accepted"])
    # the first 65 chains of the n = 130 launch are an n = 65 launch, bit for bit: another tile count, the same chains
    Y65 = dev_propose(c, cols=65)
    assert np.array_equal(_bits(Y65), _bits(Y[:, :65].contiguous()))
    a65 = dev_accept(c, Y65, cols=65)
    assert np.array_equal(_bits(a65["log_alpha"]), _bits(a["log_alpha"][:65]))
    assert np.array_equal(a65["accepted"], a["accepted"][:65])
    assert np.array_equal(_bits(a65["X"]), _bits(np.ascontiguousarray(a["X"][:, :65])))
    assert np.array_equal(_bits(a65["lp"]), _bits(a["lp"][:65]))
    if drift:
        assert np.array_equal(_bits(a65["G"]), _bits(np.ascontiguousarray(a["G"][:, :65])))


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------------------
def torch_target():
    mu, sig = _t(MU)[:, None], _t(SIGMA)[:, None]

    def log_p_t(Xt):
        X = Xt.double()
        z = (X[:4] - mu) / sig
        return -0.5 * (z * z).sum(dim=0) + KAPPA * torch.cos(X[4] - THETA0)

    def score_t(Xt):
        X = Xt.double()
        return torch.cat([-(X[:4] - mu) / (sig * sig), (-KAPPA * torch.sin(X[4] - THETA0))[None, :]]).contiguous()

    return log_p_t, score_t


@pytest.mark.parametrize("kernel", ["mala", "rw"])
def test_loop_is_the_sequence_of_binding_calls(kernel):
    log_p_t, score_t = torch_target()
    rng = np.random.RandomState(4)
    start = (T_START[:, None] + 0.1 * T_H[:, None] * rng.randn(5, 130)).astype(np.float32)
    start[2] = start[2, 0]
    h = T_H.copy()
    h[2] = 0.0                                                         # a frozen column
    Xt = _t(start)
    res = ST.metropolis_refine_t(Xt, log_p_t, score_t, 3, h, circular=T_WRAP, kernel=kernel, seed=77)
    Mt = _t(start)
    lp, G = log_p_t(Mt).clone(), score_t(Mt) if kernel == "mala" else None
    total = torch.zeros(130, dtype=torch.int64, device=DEV)
    for t in range(3):
        Yt = nh.sample_propose_t(Mt, G, h, T_WRAP, 77, t)
        la, acc = nh.sample_accept_t(Mt, Yt, G, score_t(Yt) if kernel == "mala" else None, lp, log_p_t(Yt), h, T_WRAP, 77, t)
        total += acc
    assert np.array_equal(_bits(Xt), _bits(Mt)) and np.array_equal(_bits(res["log_p"]), _bits(lp))
    assert torch.equal(res["accepts"], total) and 0 < int(total.sum()) < 3 * 130
    assert np.array_equal(_bits(Xt[2]), _bits(start[2]))
    assert np.array_equal(res["h"].cpu().numpy(), h) and res["local_steps"] == 3 and res["jump_steps"] == 0 and res["seed"] == 77
    assert np.array_equal(_bits(log_p_t(Xt)), _bits(res["log_p"]))
    # steps = 0 leaves every bit
    Zt = _t(start)
    zero = ST.metropolis_refine_t(Zt, log_p_t, score_t, 0, h, circular=T_WRAP, kernel=kernel, seed=77)
    assert np.array_equal(_bits(Zt), _bits(start)) and zero["steps"] == 0 and int(zero["accepts"].sum()) == 0
    # h moves during the warm-up and stops with it: eight steps leave the step lengths of the first four
    A, B8 = _t(start), _t(start)
    four = ST.metropolis_refine_t(A, log_p_t, score_t, 4, h, circular=T_WRAP, kernel=kernel, warmup=4, seed=77)
    eight = ST.metropolis_refine_t(B8, log_p_t, score_t, 8, h, circular=T_WRAP, kernel=kernel, warmup=4, seed=77)
    assert np.array_equal(_bits(four["h"]), _bits(eight["h"]))
    hw = eight["h"].cpu().numpy()
    assert hw[2] == 0 and np.all(hw[[0, 1, 3, 4]] != h[[0, 1, 3, 4]]) and hw[4] <= ST.WRAP_STEP_MAX
    assert np.allclose(hw[[0, 1, 3]] / h[[0, 1, 3]], hw[0] / h[0], rtol=1e-14)  # one multiplier
    # the seed rule: None draws one from numpy's global stream, a given seed touches nothing
    state = np.random.get_state()[1].copy()
    ST.metropolis_refine_t(_t(start), log_p_t, score_t, 1, h, circular=T_WRAP, kernel=kernel, seed=5)
    assert np.array_equal(state, np.random.get_state()[1])
    np.random.seed(11)
    want = int(np.random.randint(0, 2 ** 62))
    np.random.seed(11)
    assert ST.metropolis_refine_t(_t(start), log_p_t, score_t, 1, h, circular=T_WRAP, kernel=kernel)["seed"] == want


def test_known_target_on_the_device():
    """The CPU file's conditions, same n, h, steps, seed and bounds, with torch callables as the target."""
    log_p_t, score_t = torch_target()
    Xt = _t(np.repeat(T_START[:, None], T_N, axis=1).astype(np.float32))
    res = ST.metropolis_refine_t(Xt, log_p_t, score_t, T_STEPS, T_H, circular=T_WRAP, kernel="mala", seed=T_SEED)
    rate = float(res["accepts"].sum().item()) / (T_STEPS * T_N)
    print("acceptance rate %.3f" % rate)
    assert 0.2 < rate < 0.9
    X = Xt.cpu().numpy()
    assert np.all((X[4] >= -np.float32(PI)) & (X[4] < np.float32(PI)))
    assert_target_conditions(X, "device")


def test_row_major_forms():
    c = decision_case(5, 65, True)
    Y = nh.sample_propose(c["Xt"].T, c["Gx"].T, c["h"], c["wrap"], c["seed"], c["t"], device=DEV)
    assert tuple(Y.shape) == (65, 5) and np.array_equal(_bits(Y.t().contiguous()), _bits(dev_propose(c)))
    x0 = np.repeat(T_START[None, :], 64, axis=0)
    from test_sample_mcmc_cpu import target_log_p, target_score
    out = ST.metropolis_refine(x0, lambda x: target_log_p(x.T), lambda x: target_score(x.T).T, 3, T_H, circular=T_WRAP, seed=3,
                               device=DEV)
    assert out["x"].shape == (64, 5) and out["x"].dtype == np.float32 and out["accepts"].shape == (64,) and out["steps"] == 3
    assert np.array_equal(out["log_p"], target_log_p(out["x"].T.astype(np.float64))) and out["accepts"].sum() > 0


# ---- 5. the C entries' refusals; good rows next to a frozen one ------------------------------------------------------------------------------
def test_c_entries_refuse_and_frozen_rows_do_no_harm():
    lib = nh.lib()
    c = decision_case(5, 65, True)
    X, Y, Gx, Gy = _t(c["Xt"]), _t(c["Xt"]), _t(c["Gx"]), _t(c["Gy"])
    lx, ly, h = _t(c["lp_x"]), _t(c["lp_y"]), _t(c["h"])
    la, acc = torch.zeros(65, dtype=torch.float64, device=DEV), torch.zeros(65, dtype=torch.uint8, device=DEV)
    scratch = nh.sample_accept_scratch(5, 65, DEV)
    p, null, s = nh._ptr, C.c_void_p(0), nh._stream()
    seed, t = C.c_uint64(1), C.c_uint32(0)

    def prop(Xp=p(X), Yp=p(Y), rows=5, n=65, hp=p(h)):
        return lib.nfisam_sample_propose(Xp, p(Gx), Yp, rows, n, hp, null, seed, t, s)

    def acpt(Xp=p(X), Yp=p(Y), Gxp=p(Gx), Gyp=p(Gy), lxp=p(lx), lyp=p(ly), rows=5, n=65, hp=p(h), lap=p(la), ap=p(acc), sp=p(scratch)):
        return lib.nfisam_sample_accept(Xp, Yp, Gxp, Gyp, lxp, lyp, rows, n, hp, null, seed, t, lap, ap, sp, s)

    for bad in (dict(Xp=null), dict(Yp=null), dict(hp=null), dict(rows=0), dict(n=0), dict(n=65535 * 64 + 1)):
        assert prop(**bad) == nh.ERR_ARG, bad
    for bad in (dict(Xp=null), dict(Yp=null), dict(lxp=null), dict(lyp=null), dict(hp=null), dict(lap=null), dict(ap=null),
                dict(sp=null), dict(Gxp=null), dict(Gyp=null), dict(rows=0), dict(n=0), dict(n=65535 * 64 + 1)):
        assert acpt(**bad) == nh.ERR_ARG, bad
    torch.cuda.synchronize()
    assert np.array_equal(_bits(X), _bits(c["Xt"])) and np.array_equal(_bits(Y), _bits(c["Xt"])) and not la.any() and not acc.any()
    with pytest.raises(ValueError, match="both scores, or neither"):
        nh.sample_accept_t(X, Y, Gx, None, lx, ly, c["h"])
    with pytest.raises(ValueError, match="shape of the points"):
        nh.sample_accept_t(X, Y[:4].contiguous(), Gx, Gy, lx, ly, c["h"])
    with pytest.raises(ValueError, match="contiguous float64"):
        nh.sample_propose_t(X, Gx.float(), c["h"])
    with pytest.raises(ValueError, match=r"lp_x must be a contiguous float64 \[n\]"):
        nh.sample_accept_t(X, Y, Gx, Gy, lx[:64], ly, c["h"])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_accept_t(X, Y, Gx, Gy, lx.cpu(), ly, c["h"])
    with pytest.raises(ValueError, match="finite and >= 0"):
        nh.sample_propose_t(X, Gx, -c["h"] - 1.0)
    # a frozen row holding values no arithmetic could survive (inf, NaN) and a NaN score there: the other rows are unharmed
    Xn, Gn, Gyn = c["Xt"].copy(), c["Gx"].copy(), c["Gy"].copy()
    Xn[2, ::2], Xn[2, 1::2], Gn[2], Gyn[2] = np.inf, np.nan, np.nan, np.inf
    cn = dict(c, Xt=Xn, Gx=Gn, Gy=Gyn)
    Yn = dev_propose(cn)
    assert np.array_equal(_bits(Yn[2]), _bits(Xn[2]))
    assert np.array_equal(_bits(Yn[[0, 1, 3, 4]].contiguous()), _bits(dev_propose(c)[[0, 1, 3, 4]].contiguous()))
    good, odd = dev_accept(c, dev_propose(c)), dev_accept(cn, Yn)
    assert np.all(np.isfinite(odd["log_alpha"])) and np.array_equal(_bits(odd["log_alpha"]), _bits(good["log_alpha"]))
    assert np.array_equal(odd["accepted"], good["accepted"])


# ---- 6. the solver ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_range(tmp_path_factory):
    """The small range problem through its six updates, once for the tests below: (solver, the last update's samples,
    arguments): the recipe of tests/test_sample_svgd_gpu.py, trained with the fixture's own arguments, unchanged."""
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
    fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
    kwargs = json.loads(str(fx["arguments"]))
    kwargs["cuda_training"] = True
    path = tmp_path_factory.mktemp("small_range") / "factor_graph.fg"
    path.write_text(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    nodes, truth, factors = graph_file_parser(str(path), "fg", prior_cov_scale=0.1)
    steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))
    solver = NFiSAM(NFiSAMArgs(**kwargs))
    for vs, fs in steps:
        for v in vs: solver.add_node(v)
        for f in fs: solver.add_factor(f)
        solver.update_physical_and_working_graphs()
        smp = solver.incremental_inference()
    return solver, {v: np.array(smp[v]) for v in solver.elimination_ordering}, kwargs


# The default step (0.5 spreads) is for the default warm-up of 100 steps, which shrinks it to what the correlated posterior takes;
# the few steps of a test start from a step small enough to be accepted at once.
STEP = 0.02
KEYS = {"samples", "log_p", "accept_rate", "jump_accept_rate", "step_size", "steps", "warmup", "kernel", "n", "seed"}


def test_small_range_posterior_mcmc(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    n = len(smp[order[0]])
    state = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
             list(order), len(solver.physical_factors))
    ksd0 = solver.posterior_ksd(smp)["vstat"]
    for kernel in ("mala", "rw"):
        out = solver.posterior_mcmc(smp, steps=6, warmup=3, kernel=kernel, step_size=STEP, seed=9)
        assert set(out) == KEYS
        assert out["n"] == n and out["steps"] == 6 and out["warmup"] == 3 and out["kernel"] == kernel and out["seed"] == 9
        assert out["jump_accept_rate"] is None and 0.0 <= out["accept_rate"] <= 1.0
        for v in order:
            a = out["samples"][v]
            assert a.shape == (n, v.dim) and a.dtype == np.float32 and np.all(np.isfinite(a))
            assert out["step_size"][v].shape == (v.dim,) and np.all(out["step_size"][v] > 0)
        assert any(not np.array_equal(out["samples"][v], smp[v].astype(np.float32)) for v in order)
        # valid input to the other evaluations, and log_p is theirs bit for bit
        assert out["log_p"].dtype == np.float64 and np.array_equal(solver.joint_log_pdf(out["samples"]), out["log_p"])
        again = solver.posterior_mcmc(smp, steps=6, warmup=3, kernel=kernel, step_size=STEP, seed=9)
        assert all(np.array_equal(again["samples"][v], out["samples"][v]) for v in order)
        assert np.array_equal(again["log_p"], out["log_p"]) and again["accept_rate"] == out["accept_rate"]
        other = solver.posterior_mcmc(smp, steps=6, warmup=3, kernel=kernel, step_size=STEP, seed=10)
        assert any(not np.array_equal(other["samples"][v], out["samples"][v]) for v in order)
        print("kernel = %r, 6 steps: accept rate %.3f, mean log p %.4f -> %.4f, KSD V-statistic %.5g -> %.5g"
              % (kernel, out["accept_rate"], solver.joint_log_pdf(smp).mean(), out["log_p"].mean(), ksd0,
                 solver.posterior_ksd(out["samples"])["vstat"]))
    held = order[0]
    cond = solver.posterior_mcmc(smp, steps=4, warmup=2, frozen=[held], step_size=STEP, seed=9)
    assert np.array_equal(cond["samples"][held], smp[held].astype(np.float32)) and np.all(cond["step_size"][held] == 0)
    assert any(not np.array_equal(cond["samples"][v], smp[v].astype(np.float32)) for v in order[1:])
    zero = solver.posterior_mcmc(smp, steps=0, warmup=0, seed=9)
    assert zero["steps"] == 0 and zero["accept_rate"] is None and np.array_equal(zero["log_p"], solver.joint_log_pdf(smp))
    assert all(np.array_equal(zero["samples"][v], smp[v].astype(np.float32)) for v in order)
    # pure independence steps: E_p[log p / q] >= E_q[log p / q], so the moves go towards larger weights.  The chains are paired
    # before and after, so the standard error of the change of the mean is that of the per-chain differences.
    before = solver.posterior_diagnostics(smp)["log_w"]
    jump = solver.posterior_mcmc(smp, steps=4, warmup=0, independence_every=1, step_size=STEP, seed=9)
    assert jump["accept_rate"] is None and 0.0 < jump["jump_accept_rate"] <= 1.0
    assert np.array_equal(solver.joint_log_pdf(jump["samples"]), jump["log_p"])
    after = solver.posterior_diagnostics(jump["samples"])["log_w"]
    se = np.std(after - before, ddof=1) / np.sqrt(n)
    print("independence steps: accept rate %.3f, mean log p - log q %.4f -> %.4f (standard error of the change %.4f), "
          "KSD V-statistic %.5g -> %.5g" % (jump["jump_accept_rate"], before.mean(), after.mean(), se, ksd0,
                                            solver.posterior_ksd(jump["samples"])["vstat"]))
    assert after.mean() >= before.mean() - 3.0 * se
    mixed = solver.posterior_mcmc(smp, steps=4, warmup=2, independence_every=2, step_size=STEP, seed=9)
    assert mixed["accept_rate"] is not None and mixed["jump_accept_rate"] is not None
    # nothing of the solver's state or of the random streams was touched
    assert torch.equal(state[0], torch.get_rng_state()) and torch.equal(state[1], torch.cuda.get_rng_state())
    assert np.array_equal(state[2], np.random.get_state()[1]) and state[3] == random.getstate()
    assert state[4] == list(solver.elimination_ordering) and state[5] == len(solver.physical_factors)
    own = solver.posterior_mcmc(n=130, steps=2, warmup=1, step_size=STEP)
    assert own["n"] == 130 and all(own["samples"][v].shape == (130, v.dim) for v in order) and np.all(np.isfinite(own["log_p"]))
    for bad in (dict(steps=-1), dict(warmup=500), dict(step_size=0.0), dict(step_size=[0.1, 0.1]), dict(kernel="hmc"),
                dict(independence_every=-1), dict(independence_every=1.5), dict(frozen=["x"]), dict(seed=-1),
                dict(frozen=[held], independence_every=2)):
        with pytest.raises(ValueError, match="posterior_mcmc"):
            solver.posterior_mcmc(smp, **bad)
    with pytest.raises(ValueError, match="samples lack"):
        solver.posterior_mcmc({})
