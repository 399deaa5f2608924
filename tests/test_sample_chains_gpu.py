"""The chain diagnostics on the GPU (nfisam_chain_record, nfisam_chain_finish, nfisam_hip.chain_record_t / chain_finish_t, the
`record` option of utils.Statistics.metropolis_refine_t, NFiSAM.posterior_mcmc(diagnostics=True)) against the float64 numpy
restatement of tests/test_sample_chains_cpu.py: n in {1, 2, 63, 64, 65, 130} x rows in {1, 3, 5, 67} x T in {2, 4, 14, 64} (T = 14
leaves values over at every level above 0), levels at 1, 2 and the maximum; a heading's row with a pair across the +-pi seam, a
constant row, a slowly mixing row, center=None.

Bounds, none of them measured (the CPU file derives them):
  * an accumulator: within 4 (T + 16) 2^-53 sum |terms| of the restatement's (-ffp-contract=fast may fuse carry^2 + Q: equal
    bits against numpy are not promised);
  * mean, within, rhat, tau: within that bound carried through the quotients by the computed condition number;
  * everything else -- two calls, a row alone or inside a taller matrix, the chains with and without recording -- bit for bit."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_chains_cpu import (acc_bound, assert_within, finish, finish_bounds, history, max_levels, record_history, slots)
from test_sample_mcmc_cpu import MU, SIGMA
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NS, ROWS = (1, 2, 63, 64, 65, 130), (1, 3, 5, 67)


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=dtype)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def dev_record(Hd, levels, center, wrap):
    """The T record calls over the device history Hd [T, rows, n] -> the state."""
    T, rows, n = (int(s) for s in Hd.shape)
    tb = nh.chain_tables(DEV, center, wrap)
    nh.check_chain_args(rows, n, levels, T, 0, center, wrap)
    state = nh.chain_state(rows, n, levels, DEV)
    for t in range(T):
        nh.chain_record_t(state, Hd[t], t, T, levels, tables=tb, checked=True)
    return state


def dev_finish(state, levels, T, center, wrap):
    out = nh.chain_finish_t(state, int(state.shape[1]), int(state.shape[2]), levels, T, center, wrap)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. the device against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 4, 14, 64])
def test_device_matches_the_restatement(T):
    worst_acc, worst_stat = 0.0, 0.0
    for n in NS:
        for rows in ROWS:
            hist, center, wrap = history(T, rows, n)
            Hd = _t(hist)
            keep = Hd.clone()
            for levels in sorted({1, min(2, max_levels(T)), max_levels(T)}):
                state = dev_record(Hd, levels, center, wrap)
                assert tuple(state.shape) == (slots(levels), rows, n)
                ref, ref_abs = record_history(hist, levels, center, wrap)
                got = state.cpu().numpy()
                err, B = np.abs(got - ref), acc_bound(T, ref_abs)
                assert np.all(err <= B), (n, rows, levels, float(np.max(err[B > 0] / B[B > 0])))
                if (B > 0).any():
                    worst_acc = max(worst_acc, float(np.max(err[B > 0] / B[B > 0])))
                stats = dev_finish(state, levels, T, center, wrap)
                assert stats["tau"].shape == (levels, rows)
                want, bounds = finish(ref, T, levels, center, wrap), finish_bounds(ref, ref_abs, T, levels, center)
                worst_stat = max(worst_stat, assert_within(stats, want, bounds, (n, rows, levels), circular=wrap))
                heading = wrap.astype(bool)
                assert np.all((stats["mean"][heading] >= -np.pi) & (stats["mean"][heading] < np.pi))
                if rows >= 3:                                          # the constant row: no spread, 0 / 0
                    assert stats["within"][2] == 0.0 and np.isnan(stats["rhat"][2]) and np.all(np.isnan(stats["tau"][:, 2]))
                if T < 4:
                    assert np.all(np.isnan(stats["rhat"]))
                if levels != max_levels(T):
                    continue
                # two calls of the same sequence: the same bits
                again = dev_record(Hd, levels, center, wrap)
                assert np.array_equal(_bits(again), _bits(state))
                redo = dev_finish(again, levels, T, center, wrap)
                assert all(np.array_equal(_bits(redo[k]), _bits(stats[k])) for k in stats)
                # a row alone is the same bits as inside the taller matrix
                for r in sorted({1, rows - 1} - {0}) if rows > 1 else ():
                    alone = dev_record(Hd[:, r:r + 1].contiguous(), levels, center[r:r + 1], wrap[r:r + 1])
                    assert np.array_equal(_bits(alone[:, 0]), _bits(state[:, r])), (n, rows, r)
                    one = dev_finish(alone, levels, T, center[r:r + 1], wrap[r:r + 1])
                    assert all(np.array_equal(_bits(one[k][..., 0]), _bits(stats[k][..., r])) for k in stats), (n, rows, r)
            assert np.array_equal(_bits(keep), _bits(Hd))              # the points are only read
    print("T = %d: the largest |device - restatement| / bound: accumulators %.4f, statistics %.4f" % (T, worst_acc, worst_stat))


def test_center_none_means_zero():
    T, rows, n, levels = 14, 5, 65, 3
    rng = np.random.default_rng(5)
    hist = (0.3 * rng.standard_normal((T, rows, n))).astype(np.float32)
    wrap = np.array([0, 1, 0, 0, 1], dtype=np.uint8)
    hist[:, 1] += np.float32(3.0)                                      # a heading about 3 rad: wrapped deviations from 0 straddle the seam
    hist[:, 1] = np.where(hist[:, 1] >= np.float32(np.pi), hist[:, 1] - np.float32(2 * np.pi), hist[:, 1])
    state = dev_record(_t(hist), levels, None, wrap)
    ref, ref_abs = record_history(hist, levels, None, wrap)
    assert np.all(np.abs(state.cpu().numpy() - ref) <= acc_bound(T, ref_abs))
    zeros = dev_record(_t(hist), levels, np.zeros(rows), wrap)
    assert np.array_equal(_bits(zeros), _bits(state))
    stats = dev_finish(state, levels, T, None, wrap)
    assert_within(stats, finish(ref, T, levels, None, wrap), finish_bounds(ref, ref_abs, T, levels), "center=None", circular=wrap)
    same = dev_finish(zeros, levels, T, np.zeros(rows), wrap)
    assert all(np.array_equal(_bits(same[k]), _bits(stats[k])) for k in stats)
    # no flags at all
    plain = dev_record(_t(hist), levels, None, None)
    ref, ref_abs = record_history(hist, levels)
    assert np.all(np.abs(plain.cpu().numpy() - ref) <= acc_bound(T, ref_abs))
    assert_within(dev_finish(plain, levels, T, None, None), finish(ref, T, levels), finish_bounds(ref, ref_abs, T, levels), "no flags")


# ---- 2. the input is untouched; the C entries refuse cleanly ---------------------------------------------------------------------------------
def test_input_untouched_and_clean_refusal():
    lib = nh.lib()
    T, rows, n, levels = 8, 3, 65, 2
    hist, center, wrap = history(T, rows, n)
    X = _t(hist[0])
    keep = X.clone()
    state = nh.chain_state(rows, n, levels, DEV)
    nh.chain_record_t(state, X, 0, T, levels, center, wrap)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(keep), _bits(X)) and bool(state.any())
    before = state.clone()
    out = torch.zeros(3 + levels, rows, dtype=torch.float64, device=DEV)
    p, null, s = nh._ptr, C.c_void_p(0), nh._stream()

    def rec(Xp=p(X), sp=p(state), r=rows, m=n, lv=levels, t=1, TT=T):
        return lib.nfisam_chain_record(Xp, sp, r, m, lv, null, null, C.c_uint32(t), C.c_uint32(TT), s)

    def fin(sp=p(state), r=rows, m=n, lv=levels, TT=T, mp=p(out[0]), wp=p(out[1]), rp=p(out[2]), tp=p(out[3:])):
        return lib.nfisam_chain_finish(sp, r, m, lv, C.c_uint32(TT), null, null, mp, wp, rp, tp, s)

    for bad in (dict(Xp=null), dict(sp=null), dict(r=0), dict(m=0), dict(m=65535 * 64 + 1), dict(TT=7), dict(TT=0), dict(TT=1),
                dict(t=8), dict(t=100), dict(lv=0), dict(lv=4), dict(lv=17, TT=1 << 20)):
        assert rec(**bad) == nh.ERR_ARG, bad
    for bad in (dict(sp=null), dict(mp=null), dict(wp=null), dict(rp=null), dict(tp=null), dict(r=0), dict(m=0),
                dict(m=65535 * 64 + 1), dict(TT=7), dict(TT=0), dict(lv=0), dict(lv=4), dict(lv=17, TT=1 << 20)):
        assert fin(**bad) == nh.ERR_ARG, bad
    torch.cuda.synchronize()
    assert np.array_equal(_bits(before), _bits(state)) and not out.any() and np.array_equal(_bits(keep), _bits(X))
    # the bindings' own refusals on device tensors
    with pytest.raises(ValueError, match="levels"):
        nh.chain_record_t(state, X, 0, T, 4)
    with pytest.raises(ValueError, match="even"):
        nh.chain_record_t(state, X, 0, 7, levels)
    with pytest.raises(ValueError, match="state must be"):
        nh.chain_record_t(state[:, :2].contiguous(), X, 0, T, levels)
    with pytest.raises(ValueError, match="state must be"):
        nh.chain_record_t(state.float(), X, 0, T, levels)
    with pytest.raises(ValueError, match="one value per row"):
        nh.chain_record_t(state, X, 0, T, levels, center=np.zeros(2))
    with pytest.raises(ValueError, match="contiguous float32"):
        nh.chain_record_t(state, X.double(), 0, T, levels)
    with pytest.raises(ValueError, match="state must be"):
        nh.chain_finish_t(state, rows, n + 1, levels, T)
    assert np.array_equal(_bits(before), _bits(state))


# ---- 3. metropolis_refine_t with `record` ------------------------------------------------------------------------------------------------------
def gaussian_target():
    mu, sig = _t(MU)[:, None], _t(SIGMA)[:, None]
    return (lambda Xt: -0.5 * (((Xt.double() - mu) / sig) ** 2).sum(dim=0)), (lambda Xt: -(Xt.double() - mu) / (sig * sig))


def test_metropolis_refine_with_record():
    """The Gaussian target of the CPU Metropolis file, n = 256, 64 warm-up and 256 recorded steps.  The conditions were run on
    the restatement first (numpy MALA with the same warm-up rule, four seeds): R-hat 1.004 ... 1.006, tau 2.2 ... 2.7, the
    means within 2.3 of the 5 standard errors allowed; the two groups gave R-hat 61 ... 67.  The two-group call holds its step
    of 0.01 sigma with target_accept = 0.999: at the default target the warm-up would lengthen it until the groups mix."""
    n, steps, warmup, seed = 256, 320, 64, 20262
    log_p_t, score_t = gaussian_target()
    rng = np.random.default_rng(12)
    start = (MU[:, None] + SIGMA[:, None] * rng.standard_normal((4, n))).astype(np.float32)
    h = 1.2 * SIGMA
    A = _t(start)
    plain = ST.metropolis_refine_t(A, log_p_t, score_t, steps, h, warmup=warmup, seed=seed)
    assert "chains" not in plain
    # recorded about a given centre, with the history kept on the side for the restatement
    kept = []
    center = start.astype(np.float64).mean(axis=1)
    Bm = _t(start)
    rec = ST.metropolis_refine_t(Bm, log_p_t, score_t, steps, h, warmup=warmup, seed=seed, record=dict(center=center),
                                 after_step=lambda Xt, t: kept.append(Xt.clone()) if t >= warmup else None)
    assert set(rec) == set(plain) | {"chains"}
    assert np.array_equal(_bits(A), _bits(Bm)) and np.array_equal(_bits(plain["log_p"]), _bits(rec["log_p"]))
    assert torch.equal(plain["accepts"], rec["accepts"]) and np.array_equal(_bits(plain["h"]), _bits(rec["h"]))
    ch = rec["chains"]
    assert ch["T"] == 256 and ch["levels"] == 8 and ch["n"] == n and ch["tau_levels"].shape == (8, 4)
    hist = torch.stack(kept).cpu().numpy()
    assert hist.shape == (256, 4, n)
    ref, ref_abs = record_history(hist, 8, center)
    worst = assert_within(dict(ch, tau=ch["tau_levels"]), finish(ref, 256, 8, center), finish_bounds(ref, ref_abs, 256, 8, center),
                          "metropolis_refine_t")
    pick = ST.blocking_tau(ch["tau_levels"], 256, n)
    assert np.array_equal(pick["tau"], ch["tau"]) and np.array_equal(pick["ess"], ch["ess"])
    dev = np.abs(ch["mean"] - MU) / (SIGMA / np.sqrt(ch["ess"]))
    print("R-hat %s, tau %s, ess %s, resolved %s, |mean - mu| / standard error %s; device against the restatement: %.4f of the bound"
          % (ch["rhat"], ch["tau"], ch["ess"], ch["resolved"], dev, worst))
    assert np.all(ch["rhat"] < 1.1) and np.all(dev < 5.0) and np.all(ch["resolved"])
    # the default centre: the starting points' means, computed on the device -- the same statistics up to the centring
    Cm = _t(start)
    own = ST.metropolis_refine_t(Cm, log_p_t, score_t, steps, h, warmup=warmup, seed=seed, record={})
    assert np.array_equal(_bits(A), _bits(Cm))
    assert np.allclose(own["chains"]["rhat"], ch["rhat"], rtol=1e-9) and np.allclose(own["chains"]["mean"], ch["mean"], rtol=1e-12)
    # an odd count: 255 post-warm-up states, the first is not recorded
    Dm = _t(start)
    odd = ST.metropolis_refine_t(Dm, log_p_t, score_t, 40, h, warmup=11, seed=seed, record=dict(levels=2))
    assert odd["chains"]["T"] == 28 and odd["chains"]["tau_levels"].shape == (2, 4)
    # two groups 6 sigma apart that a step of 0.01 sigma cannot bring together
    side = np.where(np.arange(n) < n // 2, -3.0, 3.0)
    apart = _t((MU[:, None] + SIGMA[:, None] * side[None, :]).astype(np.float32))
    two = ST.metropolis_refine_t(apart, log_p_t, score_t, steps, 0.01 * SIGMA, warmup=warmup, seed=seed, target_accept=0.999,
                                 record={})
    print("two groups: R-hat %s, final step / sigma %s" % (two["chains"]["rhat"], two["h"].cpu().numpy() / SIGMA))
    assert np.all(two["chains"]["rhat"] > 1.5)
    # a frozen column: its mean and within are kept, the rest is NaN by the step lengths
    hz = h.copy()
    hz[1] = 0.0
    Em = _t(start)
    held = ST.metropolis_refine_t(Em, log_p_t, score_t, 24, hz, warmup=8, seed=seed, record={})["chains"]
    assert np.isnan(held["rhat"][1]) and np.isnan(held["tau"][1]) and np.isnan(held["ess"][1]) and not held["resolved"][1]
    assert np.all(np.isfinite(held["rhat"][[0, 2, 3]])) and np.isfinite(held["mean"][1]) and abs(held["within"][1]) < 1e-12


# ---- 4. the solver -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_range(tmp_path_factory):
    """The small range problem through its six updates: the recipe of tests/test_sample_mcmc_gpu.py, unchanged."""
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


STEP = 0.02                                                            # (as in the Metropolis file: accepted at once)
KEYS = {"samples", "log_p", "accept_rate", "jump_accept_rate", "step_size", "steps", "warmup", "kernel", "n", "seed"}


def test_small_range_posterior_mcmc_diagnostics(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    n = len(smp[order[0]])
    held = order[0]
    off = solver.posterior_mcmc(smp, steps=12, warmup=3, step_size=STEP, seed=9, frozen=[held])
    assert set(off) == KEYS
    on = solver.posterior_mcmc(smp, steps=12, warmup=3, step_size=STEP, seed=9, frozen=[held], diagnostics=True)
    assert set(on) == KEYS | {"diagnostics", "rhat_max", "ess_min", "recorded"}
    assert on["recorded"] == 8                                        # 9 post-warm-up states, the first left out
    assert all(np.array_equal(_bits(on["samples"][v]), _bits(off["samples"][v])) for v in order)
    assert np.array_equal(_bits(on["log_p"]), _bits(off["log_p"])) and on["accept_rate"] == off["accept_rate"]
    assert set(on["diagnostics"]) == set(order)
    for v in order:
        d = on["diagnostics"][v]
        assert set(d) == {"mean", "rhat", "tau", "ess", "resolved"}
        assert all(d[k].shape == (v.dim,) for k in d) and d["resolved"].dtype == bool and np.all(np.isfinite(d["mean"]))
        if v is held:
            assert np.all(np.isnan(d["rhat"])) and np.all(np.isnan(d["tau"])) and np.all(np.isnan(d["ess"]))
            assert not d["resolved"].any()
        else:
            assert np.all(np.isfinite(d["rhat"])) and np.all(np.isfinite(d["tau"])) and np.all(np.isfinite(d["ess"]))
            assert np.all(d["rhat"] > 0.5) and np.all(d["tau"] >= 1.0) and np.all(d["ess"] <= n * 8)
    moving = [v for v in order if v is not held]
    assert on["rhat_max"] == max(on["diagnostics"][v]["rhat"].max() for v in moving)
    assert on["ess_min"] == min(on["diagnostics"][v]["ess"].min() for v in moving)
    print("12 steps, 8 recorded: R-hat max %.3f, ess min %.1f of %d" % (on["rhat_max"], on["ess_min"], n * 8))
    assert solver.posterior_mcmc(smp, steps=11, warmup=3, step_size=STEP, seed=9, diagnostics=True)["recorded"] == 8
    assert solver.posterior_mcmc(smp, steps=7, warmup=3, step_size=STEP, seed=9, diagnostics=True)["recorded"] == 4
    with pytest.raises(ValueError, match="posterior_mcmc: at least 4 recorded states"):
        solver.posterior_mcmc(smp, steps=6, warmup=3, step_size=STEP, seed=9, diagnostics=True)
    assert set(solver.posterior_mcmc(smp, steps=6, warmup=3, step_size=STEP, seed=9)) == KEYS
