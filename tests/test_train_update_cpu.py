"""The Adam update and the early-stop bookkeeping graded in float64 -- the graders of tests/test_train_update_gpu.py, their cases and
their own tests on the CPU.  (tests/test_train_gradient_{cpu,gpu}.py grade the gradient the update consumes; read them first.)

tests/test_hip_parity.py holds the parameters after 7 - 10 steps to a 0.99 quantile of 2e-3 and a maximum of iters x lr, the loss
record to atol 5e-3 and the stop iteration to one window.  Here every element of ONE update and every decision of the stop rule
is graded on its own scale.

`adam_grade(g, m0, v0, th0, m1, v1, th1, t, cfg)` -- float32 arrays in, three ratio arrays out.  The reference is torch.optim.Adam
in float64 with default flags: exp_avg = m0, exp_avg_sq = v0, step = t - 1 loaded into its state, .grad = g, one step(); lr, beta1,
beta2 and eps are the float32 values widened (the kernel receives floats).  The six-line closed form must agree with it (rtol 1e-12).
    r_m  = |m1 - m64| / (2^-24 (beta1 |m0| + (1 - beta1) |g|) + 2^-126)
    r_v  = |v1 - v64| / (2^-24 v64 + 2^-126)
    r_th = |th1 - (th0 - u)| / (2^-24 (|th0| + |u|) + 2^-126),  u: the float64 update from the graded implementation's OWN m1, v1
Theta from the implementation's own moments is a backward-error grade: where beta1 m0 + (1 - beta1) g cancels (m0 ~ -g / 9) the
moment's rounding is a large relative error of m, which the update passes on; graded against m64 the float32 replay reads
ratios above 1e4 there (`test_theta_graded_against_m64_...`).  2^-126 covers a flushed denormal g^2.
    bounds   r_m <= 4, r_v <= 4: three or four correctly rounded operations and the rounding of 1 - beta
             r_th <= 8 max(R32, 4), R32 <= 16: R32 is the r_th of `adam_replay32`, numpy float32 operation by operation as
             `adam_coef` / `adam_update` / `one_minus_pow` of nsf_device.h have them (the hardware's exp2, sqrt and division may
             differ by an ulp); factor 8 and floor 4 are the project's convention (tests/test_train_gradient_cpu.py)
    exact    g = m0 = v0 = 0 keeps m1 = v1 = 0 and th1 == th0 bitwise (padded hidden units); beta2 = 0: v1 == fl(g g);
             beta1 = 0: m1 == g
Inputs (`adam_inputs`, P = 20000, seeded): |g| log-uniform in [1e-9, 10] with random sign (eps = 1e-8 matters only below 1e-6),
every 11th g = 0; m0 = g U(-1, 2), every 13th m0 = -g (1 - beta1) / beta1 (the cancelling one); v0 = g^2 U(0, 3); theta = 0.5 N(0, 1),
every 7th exactly 0 (there r_th is the relative error of u itself); at t = 1 the moments are 0.  Grid: six (beta1, beta2), lr 1e-3 and
0.03, sixteen t around the branch switch t ln(beta) = -0.25 of `one_minus_pow` for each beta.  The kernel's g is fl(gsum fl(1 / n)).

`bookkeeping_grade(iter_loss, state, cfg, s0, avg0)` takes an implementation's OWN float32 loss record and final state words and
replays the reference's rule (NFiSAM.py:481-491) in float64: every window that ends at a multiple e of the window in (s0, step]
has the mean nw of iter_loss[e - wnd : e]; with a previous mean avg != 0, delta = |1 - nw / avg|; delta < tol (the float32 tol widened)
stops at e.  A window with |delta64 - tol| <= 2e-5 is UNDETERMINED: either answer passes there.  The band is 3 x the derived float32
error of delta, about 6e-6: a pairwise-or-better float32 sum of up to 300 terms of one sign errs by about log2(300) 2^-24 ~ 5e-7
relative per mean (a strictly sequential one by up to (wnd + 2) 2^-24, which is what `loss_avg` itself is held to), two means, one
division and one subtraction from 1 add 4 2^-24; the rest of the 6e-6 is margin for the sequential order.  What it costs: a `<=` for `<` cannot be told outside the band
(`test_a_stop_rule_with_le_for_lt_is_not_detectable`).  Checked by `bookkeeping_problems`:
    step        the demanded stop (an undetermined window admits its own end as well), else max_iters
    stop, have_avg   as demanded; the stopping window's mean is stored too (the device closes the window before it stops)
    loss_avg    within (wnd + 2) 2^-24 mean|l| of the float64 mean of the last closed window: the any-order summation bound
    iter_loss   [step:] == 0, [:step] finite
    no stop at avg == 0.0 or before the second window; a stop exactly on max_iters satisfies budget and rule alike
Condition (a cap): at most one undetermined window per case; the seven cases of `RUN_CASES` have none under the float32 oracle and
their closest |delta - tol| is asserted to be >= 2e-4.

Planted mistakes (`ADAM_MISTAKES`, `WINDOW_MISTAKES`), each applied to the float32 replay; it APPLIES to a case when, in float64, the mistaken
coefficients (or, for the two eps placements, the mistaken update of the theta = 0 elements) differ from the right ones by more
than 2 x the case's bound x 2^-24 relative; it must then exceed its bound:
    1 t off by one (t - 1)   2 the same for t >= 50 only   3 eps inside the sqrt   4 eps added before the sqrt(bc2) division
    5 no bias correction on v   6b one_minus_pow without its x^5 term   7 the exp2 branch taken everywhere   8 m updated with beta2
    9 g not divided by n   10 the window mean over [e - wnd + 1, e]   11 the window mean dropping element 256 when wnd > 256
Mistake 6 as first proposed -- one_minus_pow without its x^7 term -- CANNOT bite: |x| <= 1/4 makes the lost term at most
x^6 / 5040 = 4.8e-8 of the series' leading term -- with its rounding the float32 replay's 1 - beta^t moves by at most 1.4 ulp -- below
every bound the convention allows (>= 32 ulp);
`test_the_series_x7_term_is_below_one_ulp` asserts that figure and that the grader does not flag it, 6b stands in for it."""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import nsf_torch as O

EPS32 = 2.0 ** -24
TINY = 2.0 ** -126
RM_MAX = RV_MAX = 4.0
R32_TH_MAX = 16.0
BAND = 2e-5
P = 20000
N_DIV = 130                                                                    # the n of g = fl(gsum fl(1 / n)) on the CPU grid
BETAS = [(0.9, 0.999), (0.0, 0.999), (0.9, 0.0), (0.5, 0.99), (0.9, 0.9999), (0.99, 0.999)]
LRS = [1e-3, 0.03]
TS = [1, 2, 3, 4, 22, 23, 24, 249, 250, 251, 1000, 2499, 2500, 2501, 10000, 100000]

Adam = namedtuple("Adam", "lr beta1 beta2 eps")
Book = namedtuple("Book", "max_iters window tol")


def adam_cfg(lr, beta1=0.9, beta2=0.999, eps=1e-8):
    return Adam(*(np.float32(v) for v in (lr, beta1, beta2, eps)))


def bound(r32):
    return 8.0 * max(float(r32), 4.0)


def _ratio(err, scale):
    err = np.asarray(err, dtype=np.float64)
    return np.where(np.isfinite(err), err / scale, np.inf)


# ------------------------------------------------------------------ Adam: references -----
def adam_closed64(g, m0, v0, th0, t, cfg, mistake=None):
    """The closed form in float64 -> (m, v, theta, u); `mistake`: one of the float64-expressible planted mistakes."""
    lr, b1, b2, eps = (float(v) for v in cfg)
    g, m0, v0, th0 = (np.asarray(a, dtype=np.float64) for a in (g, m0, v0, th0))
    tt = t - 1 if mistake == "t-1" or (mistake == "t-1 from 50" and t >= 50) else t
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (b2 if mistake == "m with beta2" else b1) * m0 + (1 - (b2 if mistake == "m with beta2" else b1)) * g
        v = b2 * v0 + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** tt, (1.0 if mistake == "no bc2" else 1 - b2 ** tt)
        u = update64(m, v, lr / bc1, math.sqrt(bc2), eps, mistake)
    return m, v, th0 - u, u


def update64(m, v, step, bc2s, eps, mistake=None):
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mistake == "eps in sqrt":
            return step * m / np.sqrt(v / (bc2s * bc2s) + eps)
        if mistake == "eps before bc2":
            return step * m / ((np.sqrt(v) + eps) / bc2s)
        return step * m / (np.sqrt(v) / bc2s + eps)


def adam_torch64(g, m0, v0, th0, t, cfg):
    """torch.optim.Adam, float64, default flags, one step from the loaded state -> (m64, v64, th64)."""
    lr, b1, b2, eps = (float(v) for v in cfg)
    p = torch.nn.Parameter(torch.from_numpy(np.array(th0, dtype=np.float64)))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(np.array(m0, dtype=np.float64)),
                        exp_avg_sq=torch.from_numpy(np.array(v0, dtype=np.float64)))
    p.grad = torch.from_numpy(np.array(g, dtype=np.float64))
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t
    return st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy(), p.detach().numpy().copy()


def adam_grade(g, m0, v0, th0, m1, v1, th1, t, cfg):
    """-> (r_m, r_v, r_th), one ratio per element (the module docstring has the scales)."""
    for a in (g, m0, v0, th0, m1, v1, th1):
        assert np.asarray(a).dtype == np.float32
    lr, b1, b2, eps = (float(v) for v in cfg)
    m64, v64, th64 = adam_torch64(g, m0, v0, th0, t, cfg)
    mc, vc, thc, _ = adam_closed64(g, m0, v0, th0, t, cfg)
    np.testing.assert_allclose(mc, m64, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(vc, v64, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(thc, th64, rtol=1e-12, atol=1e-300)
    g64, m064, th064 = (np.asarray(a, dtype=np.float64) for a in (g, m0, th0))
    r_m = _ratio(np.abs(m1 - m64), EPS32 * (b1 * np.abs(m064) + (1 - b1) * np.abs(g64)) + TINY)
    r_v = _ratio(np.abs(v1 - v64), EPS32 * v64 + TINY)
    u = update64(m1, v1, lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t), eps)
    r_th = _ratio(np.abs(th1 - (th064 - u)), EPS32 * (np.abs(th064) + np.abs(u)) + TINY)
    return r_m, r_v, r_th


# ------------------------------------------------------------------ Adam: the float32 replay
F = np.float32


def one_minus_pow32(log_b, t, mistake=None):
    """`one_minus_pow` of nsf_device.h, operation by operation."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = F(F(t) * log_b)
        if x > F(-0.25) and mistake != "exp2 everywhere":
            if mistake == "no x^7":
                p = F(1.0 / 720.0)
            else:
                p = F(F(x * F(1.0 / 5040.0)) + F(1.0 / 720.0))
            p = F(F(p * x) + F(1.0 / 120.0))
            p = F(F(p * x) + F(1.0 / 24.0)) if mistake != "no x^5" else F(1.0 / 24.0)
            p = F(F(p * x) + F(1.0 / 6.0))
            p = F(F(p * x) + F(0.5))
            p = F(F(p * x) + F(1.0))
            return F(-F(p * x))
        return F(F(1.0) - np.exp2(F(x * F(1.4426950408889634)), dtype=np.float32))


def adam_coef32(cfg, t, n, mistake=None):
    """`adam_coef` -> (step_size, inv_bc2s, inv_n); the host passes log(beta) computed in double and rounded."""
    with np.errstate(divide="ignore", invalid="ignore"):
        log_b1, log_b2 = F(np.log(np.float64(cfg.beta1))), F(np.log(np.float64(cfg.beta2)))
        tt = t - 1 if mistake == "t-1" or (mistake == "t-1 from 50" and t >= 50) else t
        bc1, bc2 = one_minus_pow32(log_b1, tt, mistake), one_minus_pow32(log_b2, tt, mistake)
        if mistake == "no bc2":
            bc2 = F(1.0)
        return F(cfg.lr / bc1), F(F(1.0) / np.sqrt(bc2, dtype=np.float32)), F(F(1.0) / F(n))


def adam_replay32(gsum, n, m0, v0, th0, t, cfg, mistake=None):
    """`adam_update` on float32 arrays -> (g, m1, v1, th1): every operation rounded on its own, as `rounded()` makes them."""
    step, inv_bc2s, inv_n = adam_coef32(cfg, t, n, mistake)
    b1, b2, eps = cfg.beta1, cfg.beta2, cfg.eps
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        g = gsum * inv_n
        ge = gsum if mistake == "g not / n" else g
        bm = b2 if mistake == "m with beta2" else b1
        m1 = bm * m0 + (F(1.0) - bm) * ge
        v1 = b2 * v0 + ((F(1.0) - b2) * ge) * ge
        if mistake == "eps in sqrt":
            denom = np.sqrt((v1 * inv_bc2s) * inv_bc2s + eps)
        elif mistake == "eps before bc2":
            denom = (np.sqrt(v1) + eps) * inv_bc2s
        else:
            denom = np.sqrt(v1) * inv_bc2s + eps
        th1 = th0 - (step * m1) / denom
    for a in (g, m1, v1, th1):
        assert a.dtype == np.float32
    return g, m1, v1, th1


@functools.lru_cache(maxsize=None)
def adam_inputs(beta1, t, seed=20240, count=P, n=N_DIV):
    """-> (gsum, g, m0, v0, th0), float32, read-only (the module docstring has the recipe); g = fl(gsum fl(1 / n))."""
    rng = np.random.RandomState(seed + 7 * t + int(1000 * beta1))
    g = np.exp(rng.uniform(math.log(1e-9), math.log(10.0), count)) * np.where(rng.rand(count) < 0.5, -1.0, 1.0)
    g[::11] = 0.0
    gsum = (g * n).astype(np.float32)
    g = gsum * F(F(1.0) / F(n))
    m0 = (g * rng.uniform(-1, 2, count)).astype(np.float32)
    if beta1 > 0:
        m0[::13] = (-g[::13].astype(np.float64) * (1 - float(F(beta1))) / float(F(beta1))).astype(np.float32)
    v0 = (g.astype(np.float64) ** 2 * rng.uniform(0, 3, count)).astype(np.float32)
    th0 = (0.5 * rng.randn(count)).astype(np.float32)
    th0[::7] = 0.0
    if t == 1:
        m0[:], v0[:] = 0.0, 0.0
    for a in (gsum, g, m0, v0, th0):
        a.setflags(write=False)
    return gsum, g, m0, v0, th0


def seeded_moments(g, beta1, t, seed):
    """Moments around a given float32 gradient g (any shape), by the recipe of `adam_inputs` -> (m0, v0) float32."""
    rng = np.random.RandomState(seed)
    g = np.asarray(g, dtype=np.float32)
    flat = g.reshape(-1)
    m0 = (flat * rng.uniform(-1, 2, flat.size)).astype(np.float32)
    if beta1 > 0:
        m0[::13] = (-flat[::13].astype(np.float64) * (1 - float(F(beta1))) / float(F(beta1))).astype(np.float32)
    v0 = (flat.astype(np.float64) ** 2 * rng.uniform(0, 3, flat.size)).astype(np.float32)
    if t == 1:
        m0[:], v0[:] = 0.0, 0.0
    return m0.reshape(g.shape), v0.reshape(g.shape)


def exact_parts(g, m0, v0, th0, m1, v1, th1, cfg):
    """The tolerance-free statements -> list of the violated ones."""
    bad = []
    z = (g == 0) & (m0 == 0) & (v0 == 0)
    if np.any(m1[z] != 0) or np.any(v1[z] != 0) or not np.array_equal(th1[z].view(np.int32), th0[z].view(np.int32)):
        bad.append("an element without gradient or moments moved")
    if cfg.beta2 == 0 and not np.array_equal(v1, g * g):
        bad.append("beta2 = 0: v1 != fl(g g)")
    if cfg.beta1 == 0 and not np.array_equal(m1, g):
        bad.append("beta1 = 0: m1 != g")
    return bad


def adam_verdict(g, m0, v0, th0, m1, v1, th1, t, cfg, r32=None, n=N_DIV):
    """Grade one update and its float32 replay on the same inputs -> dict(r_m, r_v, r_th, R32, bound, problems)."""
    r_m, r_v, r_th = adam_grade(g, m0, v0, th0, m1, v1, th1, t, cfg)
    if r32 is None:
        # the replay starts from g itself: gsum = g at n = 1 (fl(g 1) = g), so that both see the same gradient bits
        _, mr, vr, tr = adam_replay32(g, 1, m0, v0, th0, t, cfg)
        r32 = float(adam_grade(g, m0, v0, th0, mr, vr, tr, t, cfg)[2].max())
    out = dict(r_m=float(r_m.max()), r_v=float(r_v.max()), r_th=float(r_th.max()), R32=float(r32), bound=bound(r32))
    problems = list(exact_parts(g, m0, v0, th0, m1, v1, th1, cfg))
    if out["R32"] > R32_TH_MAX:
        problems.append("R32 %.2f > %g" % (out["R32"], R32_TH_MAX))
    if out["r_m"] > RM_MAX:
        problems.append("r_m %.3g > %g" % (out["r_m"], RM_MAX))
    if out["r_v"] > RV_MAX:
        problems.append("r_v %.3g > %g" % (out["r_v"], RV_MAX))
    if out["r_th"] > out["bound"]:
        problems.append("r_th %.3g > %g" % (out["r_th"], out["bound"]))
    out["problems"] = problems
    return out


# ------------------------------------------------------------------ the stop rule --------
def bookkeeping_grade(iter_loss, state, cfg, s0=0, avg0=None):
    """Replay the window rule in float64 on the implementation's own record (the module docstring has the rule) ->
    dict(stop_at: the end of the first determined window that demands a stop, or None; admitted: the steps that pass; mean64: of the
    last window closed at or before state['step'], or None; undetermined: [window ends]; closest: the smallest |delta - tol|;
    rule_fired_at: {end: delta} of every evaluated window).  Windows are replayed up to state['step'] only: the record ends there."""
    l = np.asarray(iter_loss, dtype=np.float64)
    wnd, tol, step = int(cfg.window), float(np.float32(cfg.tol)), int(state["step"])
    have, avg = avg0 is not None, (float(np.float32(avg0)) if avg0 is not None else 0.0)
    out = dict(stop_at=None, admitted=set(), mean64=None, undetermined=[], closest=np.inf, deltas={}, last_end=None)
    if wnd > 0:
        e = (s0 // wnd + 1) * wnd
        while e <= min(step, cfg.max_iters):
            assert e - wnd >= 0
            nw = float(np.mean(l[e - wnd:e]))
            if have and avg != 0.0:
                delta = abs(1.0 - nw / avg)
                out["deltas"][e] = delta
                out["closest"] = min(out["closest"], abs(delta - tol))
                if abs(delta - tol) <= BAND:
                    out["undetermined"].append(e)
                    out["admitted"].add(e)                                    # either answer passes: stop here or go on
                elif delta < tol:
                    out["stop_at"] = e
            # the stored mean is the implementation's own float32 one; the replay goes on from the float64 mean of the same window
            have, avg, out["mean64"], out["last_end"] = True, nw, nw, e
            if out["stop_at"] is not None:
                break
            e += wnd
    out["admitted"].add(out["stop_at"] if out["stop_at"] is not None else cfg.max_iters)
    out["have_avg"] = int(have)
    return out


def bookkeeping_problems(iter_loss, state, cfg, s0=0, avg0=None):
    """Everything the module docstring lists, against `bookkeeping_grade` -> (list of violated statements, the grade)."""
    il = np.asarray(iter_loss)
    assert il.dtype == np.float32
    gr = bookkeeping_grade(il, state, cfg, s0, avg0)
    step, wnd = int(state["step"]), int(cfg.window)
    bad = []
    if len(gr["undetermined"]) > 1:
        bad.append("more than one undetermined window: %s" % gr["undetermined"])
    if step not in gr["admitted"]:
        bad.append("step %d, demanded %s" % (step, sorted(gr["admitted"])))
    if gr["stop_at"] is not None and step > gr["stop_at"]:
        bad.append("ran past the demanded stop %d" % gr["stop_at"])
    stopped = gr["stop_at"] == step or (step in gr["undetermined"] and int(state["stop"]) == 1)
    if int(state["stop"]) != int(stopped):
        bad.append("stop flag %d at step %d, demanded %d" % (state["stop"], step, stopped))
    if int(state["stop"]) == 1 and (wnd <= 0 or step % wnd != 0 or step not in gr["deltas"]):
        bad.append("stopped where the rule takes no decision (avg == 0, the first window, or no window end)")
    if step > cfg.max_iters:
        bad.append("step past max_iters")
    if int(state["have_avg"]) != gr["have_avg"]:
        bad.append("have_avg %d, demanded %d" % (state["have_avg"], gr["have_avg"]))
    gr["avg_err_over_bound"] = 0.0
    if gr["mean64"] is not None:
        e = gr["last_end"]
        lim = (wnd + 2) * EPS32 * float(np.mean(np.abs(il[e - wnd:e].astype(np.float64))))
        err = abs(float(np.float32(state["loss_avg"])) - gr["mean64"])
        gr["avg_err_over_bound"] = err / lim if lim > 0 else (0.0 if err == 0 else np.inf)
        if not err <= lim:
            bad.append("loss_avg off by %.3g, bound %.3g" % (err, lim))
    elif avg0 is not None and np.float32(state["loss_avg"]) != np.float32(avg0):
        bad.append("loss_avg changed without a closed window")
    if np.any(il[step:] != 0):
        bad.append("iter_loss not 0 behind step")
    if not np.all(np.isfinite(il[:step])):
        bad.append("iter_loss not finite before step")
    return bad, gr


def bookkeep32(losses, cfg, s0=0, avg0=None, mistake=None):
    """The rule as `bookkeep_body` / the float32 oracle run it, on a FULL float32 loss record (one that never stopped) ->
    (iter_loss zero-filled behind the stop, state words).  The stopping window's mean is stored, as the device does."""
    l = np.asarray(losses, dtype=np.float32)
    wnd, tol = int(cfg.window), np.float32(cfg.tol)
    have, avg, step, stop = int(avg0 is not None), np.float32(avg0 if avg0 is not None else 0.0), cfg.max_iters, 0
    e = (s0 // wnd + 1) * wnd if wnd > 0 else cfg.max_iters + 1
    while e <= cfg.max_iters:
        lo, hi = (e - wnd + 1, min(e + 1, len(l))) if mistake == "window shifted" else (e - wnd, e)
        w = l[lo:hi]
        if mistake == "element 256 dropped" and wnd > 256:
            w = np.delete(w, 256)
        s = np.float32(0)
        for x in w:
            s = np.float32(s + x)
        nw = np.float32(s / np.float32(wnd))
        fire = False
        if have and avg != 0:
            delta = np.float32(abs(np.float32(1.0) - np.float32(nw / avg)))
            fire = delta <= tol if mistake == "le for lt" else delta < tol
        have, avg = 1, nw
        if fire:
            step, stop = e, 1
            break
        e += wnd
    il = l[:cfg.max_iters].copy()
    il[step:] = 0
    return il, dict(step=step, stop=stop, have_avg=have, loss_avg=float(avg))


# the whole runs of tests/test_train_update_gpu.py: (n, D, K, H, L, window, tol, max_iters, lr, seed)
RUN_CASES = [(96, 2, 5, 4, 1, 20, 5e-3, 600, 0.03, 5), (64, 3, 9, 8, 1, 1, 1e-3, 300, 0.02, 6), (130, 2, 5, 8, 2, 300, 2e-2, 1500, 0.02, 7),
             (100, 3, 5, 8, 1, 128, 1e-2, 1100, 0.02, 8), (70, 1, 9, 8, 1, 7, 3e-3, 500, 0.03, 9), (96, 2, 5, 4, 1, 256, 1e-2, 1500, 0.03, 10),
             (96, 2, 5, 4, 1, 257, 1e-2, 1500, 0.03, 11)]
B = 5.0
CLOSEST_MIN = 2e-4
ORACLE_UNDETERMINED = {10: [1024]}           # seed -> undetermined windows of the one-thread float32 oracle (the cap: one per case)


def run_id(rc):
    return "n%d-d%dk%dh%dl%d-w%d-s%d" % (rc[0], rc[1], rc[2], rc[3], rc[4], rc[5], rc[9])


@functools.lru_cache(maxsize=None)
def run_problem(n, D, K, H, L, seed):
    """The data recipe of `test_training_loop_early_stop_matches_oracle` -> (blob, x) float32, read-only."""
    gen = torch.Generator().manual_seed(seed)
    blob = torch.cat([O.init_blob(D, K, H, gen) for _ in range(L)]).numpy().astype(np.float32)
    x = torch.randn(n, D, generator=gen)
    if D >= 2:
        x[:, 1] = x[:, 0] ** 2 - 1 + 0.3 * x[:, 1]
    x = ((x - x.mean(0)) / x.std(0)).numpy().astype(np.float32)
    blob.setflags(write=False)
    x.setflags(write=False)
    return blob, x


@functools.lru_cache(maxsize=None)
def oracle_run(rc, early_stop=True):
    """The float32 oracle on a run case (one thread: reproducible) -> (iter_loss [max_iters], iterations run); shared, read-only."""
    n, D, K, H, L, wnd, tol, iters, lr, seed = rc
    blob, x = run_problem(n, D, K, H, L, seed)
    with CO.one_thread():
        _, il, it, _, _ = CO.train(x, blob, K, H, B, L, lr=lr, max_iters=iters, average_window=wnd, loss_delta_tol=tol,
                                   early_stop=early_stop, dtype=np.float32)
    il.setflags(write=False)
    return il, it


def oracle_state(rc):
    """The float32 oracle's run as record + state words (it keeps no loss_avg: the float32 mean of the last closed window)."""
    il, it = oracle_run(rc)
    cfg = Book(rc[7], rc[5], rc[6])
    wnd = cfg.window
    e = it // wnd * wnd
    avg = np.float32(0)
    for x in il[e - wnd:e] if e > 0 else []:
        avg = np.float32(avg + x)
    return il, dict(step=it, stop=int(it < cfg.max_iters), have_avg=int(e > 0), loss_avg=float(avg / np.float32(wnd))), cfg


# ------------------------------------------------------------------ CPU tests: Adam ------
GRID = [(b, lr, t) for b in BETAS for lr in LRS for t in TS]


def grid_id(b, lr, t):
    return "b%g-%g-lr%g-t%d" % (b[0], b[1], lr, t)


@functools.lru_cache(maxsize=None)
def replay_verdict(b, lr, t, mistake=None):
    cfg = adam_cfg(lr, *b)
    gsum, g, m0, v0, th0 = adam_inputs(b[0], t)
    _, m1, v1, th1 = adam_replay32(gsum, N_DIV, m0, v0, th0, t, cfg, mistake)
    if mistake is None:
        r32 = float(adam_grade(g, m0, v0, th0, m1, v1, th1, t, cfg)[2].max())
    else:
        r32 = replay_verdict(b, lr, t)["R32"]
    return adam_verdict(g, m0, v0, th0, m1, v1, th1, t, cfg, r32=r32)


@pytest.mark.parametrize("b", BETAS, ids=["b%g-%g" % b for b in BETAS])
def test_float32_replay_is_under_every_bound(b):
    worst = dict(r_m=0.0, r_v=0.0, R32=0.0)
    for lr in LRS:
        for t in TS:
            v = replay_verdict(b, lr, t)
            assert not v["problems"], (b, lr, t, v)
            for k in worst:
                worst[k] = max(worst[k], v[k])
    print("beta %s: float32 replay r_m %.2f  r_v %.2f  R32 %.2f" % (b, worst["r_m"], worst["r_v"], worst["R32"]))
    assert worst["r_m"] <= RM_MAX and worst["r_v"] <= RV_MAX and worst["R32"] <= R32_TH_MAX


def test_float64_update_rounded_to_float32_reads_below_one():
    for b, lr, t in [(BETAS[0], 0.03, 23), (BETAS[3], 1e-3, 250)]:
        cfg = adam_cfg(lr, *b)
        _, g, m0, v0, th0 = adam_inputs(b[0], t)
        m64, v64, _ = adam_torch64(g, m0, v0, th0, t, cfg)
        m1, v1 = m64.astype(np.float32), v64.astype(np.float32)
        th1 = (th0.astype(np.float64) - update64(m1, v1, float(cfg.lr) / (1 - float(cfg.beta1) ** t), math.sqrt(1 - float(cfg.beta2) ** t),
                                                  float(cfg.eps))).astype(np.float32)
        r_m, r_v, r_th = adam_grade(g, m0, v0, th0, m1, v1, th1, t, cfg)
        assert r_m.max() <= 1.0 and r_v.max() <= 1.0 and r_th.max() <= 1.0


def test_theta_graded_against_m64_would_read_above_1e4_where_the_moment_cancels():
    b, lr, t = BETAS[0], 0.03, 23
    cfg = adam_cfg(lr, *b)
    gsum, g, m0, v0, th0 = adam_inputs(b[0], t)
    _, m1, v1, th1 = adam_replay32(gsum, N_DIV, m0, v0, th0, t, cfg)
    _, _, th64, u64 = adam_closed64(g, m0, v0, th0, t, cfg)
    forward = _ratio(np.abs(th1 - th64), EPS32 * (np.abs(th0.astype(np.float64)) + np.abs(u64)) + TINY)
    assert forward[::13].max() > 1e4                                          # the cancelling elements, graded forward
    assert adam_grade(g, m0, v0, th0, m1, v1, th1, t, cfg)[2].max() <= R32_TH_MAX


def _applies(mistake, b, lr, t, bnd):
    """Does the mistake change, in float64, what it touches by more than 2 x bound x 2^-24 relative?  (module docstring)"""
    cfg = adam_cfg(lr, *b)
    thr = 2 * bnd * EPS32
    b1, b2 = float(cfg.beta1), float(cfg.beta2)
    if mistake in ("m with beta2", "g not / n"):
        return True
    with np.errstate(divide="ignore", invalid="ignore"):
        k64 = math.sqrt(1 - b2 ** t) / (1 - b1 ** t)                            # u is k lr m / sqrt(v) where eps does not matter
        if mistake in ("no x^7", "no x^5", "exp2 everywhere"):                # float32 effects: the mistaken replay's own coefficients
            step, inv_bc2s, _ = adam_coef32(cfg, t, N_DIV, mistake)
            k = float(step) / float(cfg.lr) / float(inv_bc2s)
            return abs(k / k64 - 1) > thr
        if mistake in ("t-1", "t-1 from 50", "no bc2"):
            tt = t - 1 if mistake == "t-1" or (mistake == "t-1 from 50" and t >= 50) else t
            if tt == 0:
                return True                                                   # a division by 0
            k = math.sqrt(1.0 if mistake == "no bc2" else 1 - b2 ** tt) / (1 - b1 ** tt)
            return abs(k / k64 - 1) > thr
        _, g, m0, v0, th0 = adam_inputs(b[0], t)
        z = (th0 == 0) & (g != 0)
        _, _, _, u = adam_closed64(g[z], m0[z], v0[z], th0[z], t, cfg)
        _, _, _, uw = adam_closed64(g[z], m0[z], v0[z], th0[z], t, cfg, mistake)
        return bool(np.nanmax(np.abs(uw - u) / np.abs(u)) > thr)


ADAM_MISTAKES = ["t-1", "t-1 from 50", "eps in sqrt", "eps before bc2", "no bc2", "no x^5", "exp2 everywhere", "m with beta2", "g not / n"]
# the fewest grid cases (of 192) each must apply to, from the grid itself: t - 1 changes 1 - beta^t by more than 1e-5 while
# beta^t > 1e-4, i.e. at least for t <= 24 (7 t x 12); from 50 on: t = 249 .. 251 at beta2 = 0.999 or 0.9999, beta1 = 0.99 (8 of the 12
# (beta, lr) x 3 t); the eps placements wherever g reaches 1e-9 (every case; `eps before bc2` and `no bc2` need bc2 != 1: beta2 > 0 and
# beta2^t > 1e-4, at least t <= 2501 at beta2 >= 0.999); the x^5 term is x^4 / 120 = 3e-5 of the series at x = -1/4: t = 2 at beta1 = 0.9
# (x = -0.21) and t = 249 - 250 at beta2 = 0.999; the exp2 branch loses 1 / |x| ulp to the cancellation in 1 - 2^x: at least beta2 =
# 0.9999 with t <= 4 (|x| <= 4e-4: thousands of ulp, unless the rounding of 2^x happens to be exact)
MIN_APPLIES = {"t-1": 84, "t-1 from 50": 24, "eps in sqrt": 192, "eps before bc2": 100, "no bc2": 100, "no x^5": 12, "exp2 everywhere": 8,
               "m with beta2": 192, "g not / n": 192}


@pytest.mark.parametrize("mistake", ADAM_MISTAKES)
def test_a_planted_adam_mistake_exceeds_its_bound_wherever_it_applies(mistake):
    applied = 0
    for b, lr, t in GRID:
        base = replay_verdict(b, lr, t)
        if not _applies(mistake, b, lr, t, base["bound"]):
            continue
        applied += 1
        v = replay_verdict(b, lr, t, mistake)
        assert v["problems"], (mistake, b, lr, t, v)
    print("%-16s applies to %3d of %d cases, flagged in each" % (mistake, applied, len(GRID)))
    assert applied >= MIN_APPLIES[mistake], applied


def test_the_series_x7_term_is_below_one_ulp():
    """Mistake 6 as proposed: the lost term is x^7 / 5040 with |x| <= 1/4 -- at most 0.25^6 / 5040 = 4.8e-8 of the leading term."""
    worst = 0.0
    for b, lr, t in GRID:
        cfg = adam_cfg(lr, *b)
        with np.errstate(divide="ignore"):
            for beta in (cfg.beta1, cfg.beta2):
                log_b = F(np.log(np.float64(beta)))
                right, wrong = one_minus_pow32(log_b, t), one_minus_pow32(log_b, t, "no x^7")
                if right != 0:
                    worst = max(worst, abs(float(wrong) - float(right)) / float(right))
        assert not _applies("no x^7", b, lr, t, bound(0.0))
        assert not replay_verdict(b, lr, t, "no x^7")["problems"]
    print("one_minus_pow without x^7: at most %.3g relative = %.2f ulp" % (worst, worst / EPS32))
    assert worst <= 2 * EPS32


def test_exact_parts_flag_a_moved_padding_element():
    b, lr, t = BETAS[0], 0.03, 4
    cfg = adam_cfg(lr, *b)
    gsum, g, m0, v0, th0 = adam_inputs(b[0], t)
    m0, v0 = m0.copy(), v0.copy()
    m0[::11], v0[::11] = 0.0, 0.0
    _, m1, v1, th1 = adam_replay32(gsum, N_DIV, m0, v0, th0, t, cfg)
    assert not exact_parts(g, m0, v0, th0, m1, v1, th1, cfg)
    th1[11] = np.nextafter(th1[11], np.float32(9))
    assert exact_parts(g, m0, v0, th0, m1, v1, th1, cfg)


# ------------------------------------------------------------------ CPU tests: the stop rule
@pytest.mark.parametrize("rc", RUN_CASES, ids=[run_id(rc) for rc in RUN_CASES])
def test_float32_oracle_stops_where_the_float64_rule_says(rc):
    il, state, cfg = oracle_state(rc)
    bad, gr = bookkeeping_problems(il, state, cfg)
    print("%-28s stop %4d  undetermined %s  closest |delta - tol| %.3g  loss_avg error / bound %.3f"
          % (run_id(rc), state["step"], gr["undetermined"], gr["closest"], gr["avg_err_over_bound"]))
    assert not bad, bad
    assert gr["undetermined"] == ORACLE_UNDETERMINED.get(rc[9], [])
    if not gr["undetermined"]:
        assert gr["closest"] >= CLOSEST_MIN
    assert state["step"] == (gr["stop_at"] if state["stop"] else cfg.max_iters)
    # the replay of the rule on the record of a run without the rule is the oracle's own
    il2, st2 = bookkeep32(oracle_run(rc, False)[0], cfg)
    assert st2["step"] == state["step"] and st2["stop"] == state["stop"] and np.array_equal(il2, il)
    assert not bookkeeping_problems(il2, st2, cfg)[0]


def _shift_applies(rc):
    """Mistake 10 applies where the shifted window's float64 mean leaves the right one by more than twice the bound of loss_avg."""
    cfg = Book(rc[7], rc[5], rc[6])
    full = oracle_run(rc, False)[0].astype(np.float64)
    e = min(bookkeep32(full, cfg)[1]["step"], len(full) - 1) // cfg.window * cfg.window
    if e >= len(full):
        e -= cfg.window
    lim = (cfg.window + 2) * EPS32 * float(np.mean(np.abs(full[e - cfg.window:e])))
    return abs(full[e] - full[e - cfg.window]) / cfg.window > 2 * lim


WINDOW_MISTAKES = [(rc, "window shifted") for rc in RUN_CASES] + [(rc, "element 256 dropped") for rc in RUN_CASES if rc[5] > 256]


@pytest.mark.parametrize("rc,mistake", WINDOW_MISTAKES, ids=["%s-%s" % (run_id(rc), m.replace(" ", "-")) for rc, m in WINDOW_MISTAKES])
def test_a_planted_window_mistake_is_flagged(rc, mistake):
    cfg = Book(rc[7], rc[5], rc[6])
    il, st = bookkeep32(oracle_run(rc, False)[0], cfg, mistake=mistake)
    bad, gr = bookkeeping_problems(il, st, cfg)
    applies = mistake == "element 256 dropped" or _shift_applies(rc)
    print("%-28s %-20s applies: %s  flagged: %s" % (run_id(rc), mistake, applies, bad))
    # a window of up to 20 iterations: 2 wnd (wnd + 2) 2^-24 <= 5.3e-5 of the loss, which a run at lr >= 0.02 moves by in every window
    assert applies or cfg.window > 20
    if applies:
        assert bad, (mistake, st, gr)


@pytest.mark.parametrize("rc", RUN_CASES, ids=[run_id(rc) for rc in RUN_CASES])
def test_a_stop_one_window_late_or_early_is_flagged(rc):
    il, state, cfg = oracle_state(rc)
    full = oracle_run(rc, False)[0]
    early = state["step"] // cfg.window * cfg.window - cfg.window                             # a window early
    while early in ORACLE_UNDETERMINED.get(rc[9], []):                                          # (an undetermined window may stop: by design)
        early -= cfg.window
    steps = [early]
    if state["stop"]:
        steps.append(min(state["step"] + cfg.window, cfg.max_iters))                            # a window late (or the budget)
    for step in steps:
        rec = full[:cfg.max_iters].copy()
        rec[step:] = 0
        e = step // cfg.window * cfg.window
        wn = np.float32(np.mean(rec[e - cfg.window:e].astype(np.float64)))
        assert bookkeeping_problems(rec, dict(step=step, stop=int(step == e), have_avg=1, loss_avg=float(wn)), cfg)[0]


def test_a_stop_rule_with_le_for_lt_is_not_detectable():
    """What the band costs: delta == tol in float32 is inside it, so `<=` for `<` passes wherever it differs."""
    for rc in RUN_CASES:
        cfg = Book(rc[7], rc[5], rc[6])
        full = oracle_run(rc, False)[0]
        il, st = bookkeep32(full, cfg, mistake="le for lt")
        assert not bookkeeping_problems(il, st, cfg)[0]
    # a record built so that the two rules differ: constant windows whose means have the ratio 1 - tol exactly in float32
    cfg = Book(40, 4, 0.25)
    full = np.array([4.0] * 4 + [3.0] * 4 + [1.0] * 32, dtype=np.float32)
    right, wrong = bookkeep32(full, cfg), bookkeep32(full, cfg, mistake="le for lt")
    assert right[1]["step"] == 16 and wrong[1]["step"] == 8                  # (delta = 1/4 = tol at 8; the flat tail stops the right rule at 16)
    for il, st in (right, wrong):
        bad, gr = bookkeeping_problems(il, st, cfg)
        assert not bad and (st["step"] != 8 or gr["undetermined"] == [8])


def test_rule_edges_of_the_grader():
    cfg = Book(12, 4, 0.1)
    flat = np.full(12, 2.0, dtype=np.float32)
    # before the second window no stop; from the second on a flat record stops at once
    il, st = bookkeep32(flat, cfg)
    assert st["step"] == 8 and not bookkeeping_problems(il, st, cfg)[0]
    first = flat.copy()
    first[4:] = 0
    assert bookkeeping_problems(first, dict(step=4, stop=1, have_avg=1, loss_avg=2.0), cfg)[0]
    # avg == 0.0: no stop, the average is updated
    il, st = bookkeep32(flat, Book(4, 4, 0.1), avg0=0.0)
    assert st["step"] == 4 and st["stop"] == 0 and st["loss_avg"] == 2.0
    assert not bookkeeping_problems(il, st, Book(4, 4, 0.1), avg0=0.0)[0]
    assert bookkeeping_problems(il, dict(st, stop=1), Book(4, 4, 0.1), avg0=0.0)[0]
    assert bookkeeping_problems(il, dict(st, loss_avg=0.0), Book(4, 4, 0.1), avg0=0.0)[0]
    # a stop exactly on max_iters: budget and rule agree on the step, the flag says the rule fired
    il, st = bookkeep32(flat[:8], Book(8, 4, 0.1))
    assert st == dict(step=8, stop=1, have_avg=1, loss_avg=2.0) and not bookkeeping_problems(il, st, Book(8, 4, 0.1))[0]
    assert bookkeeping_problems(il, dict(st, stop=0), Book(8, 4, 0.1))[0]
    # the budget ends inside a window: no decision there
    ramp = np.linspace(3, 1, 10).astype(np.float32)
    il, st = bookkeep32(ramp, Book(10, 4, 1e-3))
    assert st["step"] == 10 and st["stop"] == 0 and not bookkeeping_problems(il, st, Book(10, 4, 1e-3))[0]
    # a record that is not zero behind the stop, or not finite before it
    il, st = bookkeep32(flat, cfg)
    dirty = il.copy()
    dirty[9] = 1.0
    assert bookkeeping_problems(dirty, st, cfg)[0]
    nan = il.copy()
    nan[2] = np.nan
    assert bookkeeping_problems(nan, st, cfg)[0]
