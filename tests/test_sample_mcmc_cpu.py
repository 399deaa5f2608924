"""The Metropolis kernels' host side (csrc/sample_mcmc.hip: nfisam_sample_propose / nfisam_sample_accept, nfisam_hip's bindings,
utils.Statistics.metropolis_refine, NFiSAM.posterior_mcmc) with no device, and the float64 numpy RESTATEMENT of the two kernels
-- `propose`, `accept`, `chain` -- that tests/test_sample_mcmc_gpu.py grades the device against:

  1. the new names are exported and declared;
  2. bad input is refused with no device: the bindings, `check_metropolis_options`, `posterior_mcmc` before a graph exists;
  3. the generator: the Random123 known answers through the restatement's counter layout, u strictly inside (0, 1);
  4. the restatement alone on a known target (four Gaussian columns of different spreads and one wrapped von Mises column):
     the ensemble's moments within bounds derived from n, and the same run with the accept step forced to "always" MISSES the
     variance bound -- the check can see a broken correction;
  5. the decision fixture: the cases of the GPU comparison, none of whose chains is within the rounding bound of its decision.
"""
import os
import re

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from oracle.clique_sim_ref import philox4x32_10
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI, TWO_PI = np.pi, 2.0 * np.pi
SLAB = nh.MCMC_SLAB
NEW = ("nfisam_sample_propose", "nfisam_sample_accept", "nfisam_sample_accept_scratch_count")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def uniforms(seed, chain, word, t, tag):
    """The four float64 uniforms of counter (chain, word, t, tag) under `seed`: (word + 0.5) 2^-32.  Arrays broadcast."""
    seed = int(seed)
    words = philox4x32_10((chain, word, t, tag), (seed & 0xFFFFFFFF, seed >> 32))
    return [(w.astype(np.float64) + 0.5) * 2.0 ** -32 for w in words]


def normals(seed, x_rows, n, t):
    """Z [x_rows, n]: Box-Muller (cos, sin) of (u0, u1) -> rows 4g, 4g + 1 and of (u2, u3) -> rows 4g + 2, 4g + 3."""
    G = (x_rows + 3) // 4
    u = uniforms(seed, np.arange(n, dtype=np.uint64)[None, :], np.arange(G, dtype=np.uint64)[:, None], t, 0)
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    ta, tb = TWO_PI * u[1], TWO_PI * u[3]
    Z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1)       # [G, 4, n]
    return Z.reshape(4 * G, n)[:x_rows]


def accept_uniform(seed, n, t):
    return uniforms(seed, np.arange(n, dtype=np.uint64), 0, t, 1)[0]


def wrap_pi(v):
    m = np.fmod(v + PI, TWO_PI)
    m = np.where(m < 0, m + TWO_PI, m)
    return m - PI


def signed_wrap(d):
    m = wrap_pi(np.abs(d))
    return np.where(d < 0, -m, m)


def round_point(v, wrapped):
    """float64 -> the float32 the kernels store: a wrapped value that rounds to +-float32(pi) becomes the float32 inside -pi."""
    f = v.astype(np.float32)
    g = wrap_pi(v).astype(np.float32)
    g = np.where((g.astype(np.float64) < PI) & (g.astype(np.float64) >= -PI), g, np.float32(-3.1415925)).astype(np.float32)
    g = np.where(np.isnan(v), f, g)
    return np.where(wrapped, g, f).astype(np.float32)


def propose(Xt, Gx, h, wrap, seed, t):
    """Yt [x_rows, n] float32: y = x + h z (+ (h^2 / 2) g), float64; a row with h == 0 is Xt's bits."""
    Xt = np.asarray(Xt, dtype=np.float32)
    x_rows, n = Xt.shape
    h = np.asarray(h, dtype=np.float64)[:, None]
    w = np.zeros((x_rows, 1), dtype=bool) if wrap is None else np.asarray(wrap, dtype=bool)[:, None]
    v = Xt.astype(np.float64) + h * normals(seed, x_rows, n, t)
    if Gx is not None:
        v = v + (0.5 * h * h) * np.asarray(Gx, dtype=np.float64)
    return np.where(h != 0, round_point(v, np.broadcast_to(w, v.shape)), Xt).astype(np.float32)


def accept(Xt, Yt, Gx, Gy, lp_x, lp_y, h, wrap, seed, t, always=False):
    """The accept step on COPIES -> dict(log_alpha, accepted, log_u, abs_sum (the sum of |every addend| of log alpha, the lp
    included: what the rounding bound B scales with), X, G, lp: the state after the step).  The row sum is taken in the kernel's
    order: a wave's 8 rows ascending, the four waves of a slab in order, the slabs in order."""
    Xt, Yt = np.asarray(Xt, dtype=np.float32), np.asarray(Yt, dtype=np.float32)
    x_rows, n = Xt.shape
    h = np.asarray(h, dtype=np.float64)
    lp_x, lp_y = np.asarray(lp_x, dtype=np.float64), np.asarray(lp_y, dtype=np.float64)
    total, abs_sum = np.zeros(n), np.abs(lp_x) + np.abs(lp_y)
    if Gx is not None:
        for s0 in range(0, x_rows, SLAB):
            waves = []
            for w in range(4):
                s = np.zeros(n)
                for r in range(s0 + w * SLAB // 4, min(s0 + (w + 1) * SLAB // 4, x_rows)):
                    if not h[r] > 0:
                        continue
                    d = Xt[r].astype(np.float64) - Yt[r].astype(np.float64)
                    if wrap is not None and wrap[r]:
                        d = signed_wrap(d)
                    a = 0.5 * h[r] * h[r]
                    rev, fwd = (d - a * Gy[r]) / h[r], (-d - a * Gx[r]) / h[r]
                    s = s + (0.5 * (fwd * fwd) - 0.5 * (rev * rev))
                    abs_sum = abs_sum + 0.5 * (fwd * fwd) + 0.5 * (rev * rev)
                waves.append(s)
            total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    with np.errstate(invalid="ignore"):
        log_alpha = (lp_y - lp_x) + total
    log_u = np.log(accept_uniform(seed, n, t))
    with np.errstate(invalid="ignore"):
        acc = (log_u < log_alpha) & (lp_y != -np.inf)
    if always:
        acc = np.ones(n, dtype=bool)
    X, lp = np.where(acc[None, :], Yt, Xt), np.where(acc, lp_y, lp_x)
    G = None if Gx is None else np.where(acc[None, :], Gy, Gx)
    return dict(log_alpha=log_alpha, accepted=acc.astype(np.uint8), log_u=log_u, abs_sum=abs_sum, X=X, G=G, lp=lp)


def rounding_bound(x_rows, abs_sum):
    """B = 4 (x_rows + 16) 2^-53 (sum |terms| + |lp_x| + |lp_y|): x_rows + 2 additions and a handful of roundings per term, each
    at most 2^-53 of the magnitudes added, times 4 for the two implementations' different but equally valid orders of rounding."""
    return 4.0 * (x_rows + 16) * 2.0 ** -53 * abs_sum


def chain(X0t, log_p, score, h, wrap, steps, seed, kernel="mala", always=False):
    """`steps` Metropolis steps of the restatement from X0t [D, n] -> (Xt float32, per-chain accept counts)."""
    Xt = np.asarray(X0t, dtype=np.float32).copy()
    lp = log_p(Xt.astype(np.float64))
    G = score(Xt.astype(np.float64)) if kernel == "mala" else None
    count = np.zeros(Xt.shape[1], dtype=np.int64)
    for t in range(steps):
        Yt = propose(Xt, G, h, wrap, seed, t)
        lp_y = log_p(Yt.astype(np.float64))
        Gy = score(Yt.astype(np.float64)) if kernel == "mala" else None
        out = accept(Xt, Yt, G, Gy, lp, lp_y, h, wrap, seed, t, always=always)
        Xt, G, lp = out["X"], out["G"], out["lp"]
        count += out["accepted"]
    return Xt, count


# ---- the known target: four Gaussian columns of different spreads and one von Mises column across the seam -------------------------
MU = np.array([1.0, -20.0, 0.25, 100.0])
SIGMA = np.array([0.5, 2.0, 0.05, 8.0])
KAPPA, THETA0 = 25.0, 3.0                                             # the heading's mass straddles +-pi
T_N, T_STEPS, T_SEED = 2048, 300, 20261
T_WRAP = np.array([0, 0, 0, 0, 1], dtype=np.uint8)


def _bessel_ratio(k, kappa):
    t = (np.arange(200000) + 0.5) * (PI / 200000)
    w = np.exp(kappa * (np.cos(t) - 1.0))
    return float((w * np.cos(k * t)).sum() / w.sum())                 # I_k(kappa) / I_0(kappa)


RHO, ALPHA2 = _bessel_ratio(1, KAPPA), _bessel_ratio(2, KAPPA)
T_SPREAD = np.concatenate([SIGMA, [np.sqrt(-2.0 * np.log(RHO))]])     # the circular standard deviation of the heading
T_H = 1.2 * T_SPREAD
T_START = np.concatenate([MU + 5.0 * SIGMA, [THETA0 - 1.0]])          # every chain starts at one far point


def target_log_p(X):
    z = (X[:4] - MU[:, None]) / SIGMA[:, None]
    return -0.5 * (z * z).sum(axis=0) + KAPPA * np.cos(X[4] - THETA0)


def target_score(X):
    return np.concatenate([-(X[:4] - MU[:, None]) / (SIGMA ** 2)[:, None], -KAPPA * np.sin(X[4] - THETA0)[None, :]])


def target_deviations(Xt):
    """The four conditions as (deviation / bound) arrays, every bound derived from n: the mean within 5 sigma / sqrt(n), the
    variance within 5 sqrt(2 / n) relative, the circular mean and the resultant length within 5 standard errors
    (Mardia & Jupp 4.8: var(mean direction) = (1 - alpha2) / (2 n rho^2), var(R) = (1 + alpha2 - 2 rho^2) / (2 n))."""
    X = np.asarray(Xt, dtype=np.float64)
    n = X.shape[1]
    mean = np.abs(X[:4].mean(axis=1) - MU) / (5.0 * SIGMA / np.sqrt(n))
    var = np.abs(X[:4].var(axis=1, ddof=1) / SIGMA ** 2 - 1.0) / (5.0 * np.sqrt(2.0 / n))
    c, s = np.cos(X[4]).mean(), np.sin(X[4]).mean()
    cmean = abs(wrap_pi(np.arctan2(s, c) - THETA0)) / (5.0 * np.sqrt((1.0 - ALPHA2) / (2.0 * n * RHO ** 2)))
    res = abs(np.hypot(c, s) - RHO) / (5.0 * np.sqrt((1.0 + ALPHA2 - 2.0 * RHO ** 2) / (2.0 * n)))
    return dict(mean=mean, var=var, circular_mean=np.array([cmean]), resultant=np.array([res]))


def assert_target_conditions(Xt, what):
    dev = target_deviations(Xt)
    for k, v in dev.items():
        print("%s: %s deviation / bound = %s" % (what, k, np.array2string(v, precision=3)))
    for k, v in dev.items():
        assert np.all(v < 1.0), (what, k, v)


# ---- the decision fixture: the cases of the GPU comparison ---------------------------------------------------------------------------
CASE_N = (1, 2, 63, 64, 65, 130)
CASE_ROWS = (1, 3, 4, 5, 67, SLAB - 1, SLAB, SLAB + 1)


def decision_case(x_rows, n, drift, seed=None):
    """One comparison case -> dict(Xt, Gx, Gy, lp_x, lp_y, h, wrap, seed, t).  Rows r = 1 mod 3 are angles, the first two of
    their chains a pair across the +-pi seam (x_rows == 4: no wrap array at all); rows r = 2 mod 5 are frozen.  Gy, lp_x, lp_y
    are synthetic: the accept step does not care where they come from."""
    k = CASE_ROWS.index(x_rows) * len(CASE_N) + CASE_N.index(n)
    seed = 7000 + 2 * k + int(drift) if seed is None else seed
    rng = np.random.RandomState(seed)
    spread = 10.0 ** rng.uniform(-2, 1, x_rows)
    wrap = (np.arange(x_rows) % 3 == 1) if x_rows != 4 else np.zeros(x_rows, dtype=bool)
    if x_rows == 1:
        wrap[0] = bool(k % 2)
    spread[wrap] = rng.uniform(0.02, 0.25, int(wrap.sum()))
    Xt = (rng.uniform(-50, 50, (x_rows, 1)) + spread[:, None] * rng.randn(x_rows, n)).astype(np.float32)
    ang = wrap_pi(rng.uniform(-PI, PI, (x_rows, 1)) + spread[:, None] * rng.randn(x_rows, n))
    ang[:, 0] = PI - 1e-3
    if n > 1:
        ang[:, 1] = -PI + 1e-3
    Xt[wrap] = ang[wrap].astype(np.float32)
    h = 0.8 * spread
    h[np.arange(x_rows) % 5 == 2] = 0.0
    Gx = rng.randn(x_rows, n) / spread[:, None] if drift else None
    Gy = rng.randn(x_rows, n) / spread[:, None] if drift else None
    lp_x = 50.0 * rng.randn(n)
    lp_y = lp_x + 2.0 * rng.randn(n) + (0.5 * x_rows if drift else 0.0)
    return dict(Xt=Xt, Gx=Gx, Gy=Gy, lp_x=lp_x, lp_y=lp_y, h=h, wrap=wrap.astype(np.uint8) if x_rows != 4 else None,
                seed=(seed * 0x9E3779B97F4A7C15) & ((1 << 64) - 1), t=k)


def decision_cases(drift):
    return [decision_case(r, n, drift) for r in CASE_ROWS for n in CASE_N]


def assert_decidable(case, out):
    """No chain's decision lies within the rounding bound: |log alpha - log u| > B (+ the few ulps of log u itself)."""
    B = rounding_bound(case["Xt"].shape[0], out["abs_sum"]) + 4.0 * 2.0 ** -53 * np.abs(out["log_u"])
    margin = np.abs(out["log_alpha"] - out["log_u"])
    assert np.all(np.isfinite(out["log_alpha"])) and np.all(margin > B), (case["Xt"].shape, float((margin / B).min()))


# ---- 1. exports ---------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nfisam_[a-z0-9_]+)\s*\(", hdr))
    nh.build()
    lib = nh.lib()
    for name in NEW:
        assert name in nh.EXPORTS and name in declared and hasattr(lib, name), name
    for name in ("check_mcmc_args", "sample_propose_t", "sample_accept_t", "sample_accept_scratch", "mcmc_tables", "sample_propose"):
        assert callable(getattr(nh, name)), name
    for name in ("check_metropolis_options", "metropolis_refine_t", "metropolis_refine"):
        assert callable(getattr(ST, name)), name
    assert lib.nfisam_abi_version() == 1600
    mk = open(os.path.join(ROOT, "nf-isam_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SAMPLE\s*:=.*\bsample_mcmc\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "nf-isam_amd", "csrc", "sample_mcmc.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["sample_common.h"]
    assert "atomic" not in re.sub(r"//.*", "", src)
    # the scratch count is host arithmetic: one partial per (slab of rows, chain) and the lp difference
    for rows, n in ((1, 1), (SLAB, 65), (SLAB + 1, 500), (2400, 500)):
        assert int(lib.nfisam_sample_accept_scratch_count(rows, n)) == ((rows + SLAB - 1) // SLAB + 1) * n
    assert int(lib.nfisam_sample_accept_scratch_count(0, 5)) == 0 and int(lib.nfisam_sample_accept_scratch_count(5, 0)) == 0
    assert int(lib.nfisam_sample_accept_scratch_count(5, 65535 * 64 + 1)) == 0


# ---- 2. refusals with no device ------------------------------------------------------------------------------------------------------
def test_bindings_refuse_bad_arguments_with_no_device():
    ok = dict(x_rows=3, n=4, h=[0.1, 0.0, 2.0])
    nh.check_mcmc_args(**ok)
    nh.check_mcmc_args(wrap=[0, 1, 0], seed=(1 << 64) - 1, t=(1 << 32) - 1, **ok)
    for bad, match in ((dict(h=[0.1, -1.0, 2.0]), "finite and >= 0"), (dict(h=[0.1, np.nan, 2.0]), "finite and >= 0"),
                       (dict(h=[0.1, np.inf, 2.0]), "finite and >= 0"), (dict(h=[0.1, 0.2]), "one value per row"),
                       (dict(h=None), "one value per row"), (dict(wrap=[1, 0]), "one flag per row"), (dict(seed=-1), "seed"),
                       (dict(seed=1 << 64), "seed"), (dict(seed=1.5), "seed"), (dict(t=-1), "t must"), (dict(t=1 << 32), "t must"),
                       (dict(n=0), "chains"), (dict(x_rows=0, h=[]), "rows"), (dict(n=65535 * 64 + 1), "chains")):
        with pytest.raises(ValueError, match=match):
            nh.check_mcmc_args(**dict(ok, **bad))
    X, G, lp = torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_propose_t(X, G, ok["h"])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_accept_t(X, X.clone(), G, G.clone(), lp, lp.clone(), ok["h"])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sample_propose(np.zeros((4, 3)), None, ok["h"], device="cpu")
    with pytest.raises(ValueError, match="finite and >= 0"):
        nh.sample_propose(np.zeros((4, 3)), None, [1.0, -1.0, 1.0], device="cuda")
    with pytest.raises(ValueError, match="shape of the points"):
        nh.sample_propose(np.zeros((4, 3)), np.zeros((4, 2)), ok["h"], device="cuda")


def test_check_metropolis_options():
    opt = ST.check_metropolis_options(3, 10, [0.1, 0.0, 0.2], circular=[0, 0, 1], kernel="rw", warmup=4, seed=5)
    assert opt["steps"] == 10 and opt["warmup"] == 4 and opt["target"] == 0.234 and opt["seed"] == 5 and opt["every"] == 0
    assert np.array_equal(opt["h"], [0.1, 0.0, 0.2]) and np.array_equal(opt["flags"], [False, False, True])
    assert ST.check_metropolis_options(2, 0, 0.5)["target"] == 0.574 and ST.check_metropolis_options(2, 0, 0.5)["seed"] is None
    assert ST.check_metropolis_options(2, 4, 0.5, independence=(2, lambda n, t: None))["every"] == 2
    ok = dict(width=3, steps=10, step_size=0.1)
    for bad, match in ((dict(kernel="hmc"), "kernel must be"), (dict(steps=-1), "steps must be an integer"),
                       (dict(steps=1.5), "steps must be an integer"), (dict(warmup=-1), "warmup must be an integer"),
                       (dict(warmup=11), "cannot exceed"), (dict(step_size=-0.1), "step_size"), (dict(step_size=np.inf), "step_size"),
                       (dict(step_size=[0.1, 0.1]), "step_size"), (dict(step_size="a"), "step_size"),
                       (dict(circular=[1]), "circular: one flag per column"),
                       (dict(step_size=0.31, circular=[0, 1, 0]), "nearest-image bound"),
                       (dict(target_accept=0.0), "target_accept"), (dict(target_accept=1.0), "target_accept"),
                       (dict(seed=-3), "seed"), (dict(seed=0.5), "seed"), (dict(independence=3), "independence"),
                       (dict(independence=(0, len)), "independence"), (dict(independence=(2, None)), "independence"),
                       (dict(step_size=[0.1, 0.0, 0.1], independence=(2, len)), "frozen"), (dict(width=0), "one column")):
        with pytest.raises(ValueError, match=match):
            ST.check_metropolis_options(**dict(ok, **bad))
        if "width" not in bad:
            with pytest.raises(ValueError, match=match):       # the options are refused before the CPU tensor is
                ST.metropolis_refine_t(torch.zeros(3, 6), len, len, **{k: v for k, v in dict(ok, **bad).items() if k != "width"})
    run = dict(steps=3, step_size=0.1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.metropolis_refine_t(torch.zeros(3, 6), len, len, **run)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.metropolis_refine(np.zeros((6, 3)), len, len, device="cpu", **run)
    with pytest.raises(ValueError, match="callable"):
        ST.metropolis_refine_t(torch.zeros(3, 6), None, len, **run)
    with pytest.raises(ValueError, match="callable"):
        ST.metropolis_refine_t(torch.zeros(3, 6), len, None, **run)
    with pytest.raises(ValueError, match="log_q_t"):
        ST.metropolis_refine_t(torch.zeros(3, 6), len, len, independence=(1, len), **run)
    with pytest.raises(ValueError, match="callable"):
        ST.metropolis_refine(np.zeros((6, 3)), None, len, **run)


def test_posterior_mcmc_refuses_before_a_graph_exists():
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.ParallelNFiSAM import ParallelNFiSAM
    from slam.ReplicaNFiSAM import _ReplicaSolver
    solver = NFiSAM(NFiSAMArgs())
    with pytest.raises(RuntimeError, match="posterior_mcmc: no factor graph yet"):
        solver.posterior_mcmc()
    with pytest.raises(RuntimeError, match="posterior_mcmc: no factor graph yet"):
        solver.posterior_mcmc({}, steps=3, kernel="rw", independence_every=2, seed=1)
    assert ParallelNFiSAM.posterior_mcmc is NFiSAM.posterior_mcmc and _ReplicaSolver.posterior_mcmc is NFiSAM.posterior_mcmc


# ---- 3. the generator ----------------------------------------------------------------------------------------------------------------
def test_generator_known_answers_through_the_counter_layout():
    """The Random123 known-answer vectors of Philox4x32-10 with the words where the contract puts them: counter (chain, row >> 2,
    step, tag), key (seed & 0xffffffff, seed >> 32); u = (word + 0.5) 2^-32."""
    for (chain_, word, t, tag), seed, out in (
            ((0, 0, 0, 0), 0, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ((0xffffffff,) * 4, (1 << 64) - 1, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0x299f31d0 << 32) | 0xa4093822,
             "d16cfe09 94fdcceb 5001e420 24126ea1")):
        u = uniforms(seed, chain_, word, t, tag)
        want = [int(w, 16) for w in out.split()]
        assert [float(x[0]) for x in u] == [(w + 0.5) * 2.0 ** -32 for w in want]
    # the extremes of a word: strictly inside (0, 1), and exact in float64
    for w in (0, 1, 0xffffffff):
        u = (np.float64(w) + 0.5) * 2.0 ** -32
        assert 0.0 < u < 1.0 and u * 2.0 ** 33 == 2 * w + 1
    u = uniforms(12345, np.arange(4096, dtype=np.uint64), 7, 3, 0)
    assert all(np.all((x > 0) & (x < 1)) for x in u)


def test_a_chains_draws_do_not_depend_on_n_and_differ_by_step_seed_and_tag():
    Z130, Z65 = normals(99, 67, 130, 4), normals(99, 67, 65, 4)
    assert np.array_equal(Z130[:, :65], Z65)
    assert np.array_equal(normals(99, 5, 65, 4), Z65[:5])                       # ... nor on the number of rows
    assert not np.array_equal(normals(99, 67, 65, 5), Z65) and not np.array_equal(normals(98, 67, 65, 4), Z65)
    assert not np.array_equal(accept_uniform(99, 65, 4), uniforms(99, np.arange(65, dtype=np.uint64), 0, 4, 0)[0])
    Z = normals(7, 8, 200000, 0)
    assert abs(Z.mean()) < 5.0 / np.sqrt(Z.size) and abs(Z.var() - 1.0) < 5.0 * np.sqrt(2.0 / Z.size)
    assert np.all(np.abs(np.corrcoef(Z)[np.triu_indices(8, 1)]) < 5.0 / np.sqrt(200000))


# ---- 4. the restatement alone on the known target -------------------------------------------------------------------------------------
def test_restatement_samples_the_known_target_and_an_uncorrected_chain_does_not():
    X0 = np.repeat(T_START[:, None], T_N, axis=1)
    Xt, count = chain(X0, target_log_p, target_score, T_H, T_WRAP, T_STEPS, T_SEED)
    rate = count.mean() / T_STEPS
    print("acceptance rate %.3f" % rate)
    assert 0.2 < rate < 0.9
    assert np.all((Xt[4] >= -np.float32(PI)) & (Xt[4] < np.float32(PI)))
    assert (Xt[4] > 0).any() and (Xt[4] < 0).any()                              # the heading's mass lies on both sides of the seam
    assert_target_conditions(Xt, "restatement")
    # the same run, every proposal accepted: the unadjusted chain's variance is sigma^2 / (1 - h^2 / 4 sigma^2) = 1.5625 sigma^2
    Ut, _ = chain(X0, target_log_p, target_score, T_H, T_WRAP, T_STEPS, T_SEED, always=True)
    dev = target_deviations(Ut)
    print("always accepted: variance deviation / bound = %s" % np.array2string(dev["var"], precision=3))
    assert np.all(dev["var"] > 1.0)
    ratio = Ut[:4].astype(np.float64).var(axis=1, ddof=1) / SIGMA ** 2
    assert np.all(np.abs(ratio / 1.5625 - 1.0) < 5.0 * np.sqrt(2.0 / T_N))


def test_restatement_rules():
    """Frozen rows, the special values, steps that change nothing."""
    c = decision_case(5, 65, True)
    Yt = propose(c["Xt"], c["Gx"], c["h"], c["wrap"], c["seed"], c["t"])
    assert np.array_equal(Yt[2].view(np.uint32), c["Xt"][2].view(np.uint32)) and c["h"][2] == 0
    assert np.all(Yt[[0, 1, 3, 4]] != c["Xt"][[0, 1, 3, 4]])
    assert np.all((Yt[[1, 4]] >= -np.float32(PI)) & (Yt[[1, 4]] < np.float32(PI)))
    lp_y = c["lp_y"].copy()
    lp_x = c["lp_x"].copy()
    lp_y[0], lp_x[1], lp_y[2], lp_x[3], lp_y[3] = -np.inf, -np.inf, np.nan, -np.inf, -np.inf
    out = accept(c["Xt"], Yt, c["Gx"], c["Gy"], lp_x, lp_y, c["h"], c["wrap"], c["seed"], c["t"])
    assert list(out["accepted"][:4]) == [0, 1, 0, 0]
    assert np.array_equal(out["X"][:, 1], Yt[:, 1]) and np.array_equal(out["X"][:, 0], c["Xt"][:, 0])
    assert out["lp"][1] == lp_y[1] and out["lp"][0] == lp_x[0]
    # the seam: a proposal on the other side of +-pi is a short move, not one of 2 pi
    d = signed_wrap(np.array([PI - 1e-3 - (-PI + 1e-3), -PI + 1e-3 - (PI - 1e-3), 0.5, -0.5]))
    assert np.allclose(d, [-2e-3, 2e-3, 0.5, -0.5], atol=1e-15) and np.array_equal(signed_wrap(-d), -signed_wrap(d))
    assert round_point(np.array([PI - 1e-9]), np.array([True]))[0] == np.float32(-3.1415925)


# ---- 5. the decision fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", [True, False])
def test_decision_fixture_leaves_no_chain_undecidable(drift):
    both = np.zeros(2, dtype=np.int64)
    seam = 0
    for c in decision_cases(drift):
        Yt = propose(c["Xt"], c["Gx"], c["h"], c["wrap"], c["seed"], c["t"])
        out = accept(c["Xt"], Yt, c["Gx"], c["Gy"], c["lp_x"], c["lp_y"], c["h"], c["wrap"], c["seed"], c["t"])
        assert_decidable(c, out)
        both += np.bincount(out["accepted"], minlength=2)
        if c["wrap"] is not None and c["wrap"].any():
            r = np.flatnonzero(c["wrap"] & (c["h"] > 0))
            seam += int((np.abs(Yt[r].astype(np.float64) - c["Xt"][r]) > PI).sum())
    print("accepted %d, rejected %d, proposals across the seam %d" % (both[1], both[0], seam))
    assert both.min() > 200 and seam > 10                              # both decisions and the seam are well populated
