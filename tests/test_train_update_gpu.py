"""The Adam update, the loss record and the stop rule of the training launches graded in float64: the graders, the bounds and the
run cases of tests/test_train_update_cpu.py (read its docstring first).

    r_m <= 4, r_v <= 4, r_th <= 8 max(R32, 4) over EVERY element of the kernel layout (padding included: it must not move), R32 <= 16:
    the float32 replay's ratio on the same gradient and moments; the stop rule replayed in float64 on the device's own loss record.

What is graded:
  one step       `TrainBatch.step()` from a seeded mid-run state -- moments written around the batch's own gradient (half of them
                 scaled down per element by up to 1e-6, so that eps takes part), state.step = t - 1 -- over six (beta1, beta2) x sixteen t
                 at lr = 0.03; the gradient g is the first moment of a twin batch at beta1 = beta2 = 0 (two twins agree bit for bit).
                 Shapes (n, D, K, H, L): (96,2,5,4,1) (130,5,9,8,1) (64,3,9,5,1: H padded to 8) (100,3,5,16,2: the panel image), the
                 ragged batch (129,3) (1,5) (64,2) at K = 9, H = 8, and the trained flow `trained3` of tests/golden/sampler_flows.npz.
                 Forms: default, NFISAM_FUSED_ADAM=0, at L = 2 also NFISAM_PAIR_IMAGE=0.  (`step()` closes a chunk of ONE iteration:
                 in every form the update is the Adam kernel's; the sites fused into the training kernels run inside longer chunks
                 and are held to the Adam kernel's bits by `test_fused_adam_launches_equal_the_separate_adam_kernel_bit_for_bit`
                 of tests/test_hip_parity.py.)
  a chain        twelve consecutive `step()` calls from step 0, 244 and 122 (the loss ring wraps at 128): every transition graded as
                 above against a twin that gets the snapshot's parameters; state.step advances by one; iter_loss[s] is the float64 NLL
                 of the pre-update snapshot under `loss_ratio` / `bound` of tests/test_train_gradient_cpu.py; a call at
                 step == max_iters changes no bit
  whole runs     the seven `RUN_CASES` through `run(use_graph=True)`, `run(use_graph=False)` and (L = 1) `launch_async()`, a ragged
                 batch of three, the budget edge max_iters = 610 at window 20, and seeded rule edges (have_avg = 1 with loss_avg = 0.0;
                 loss_avg = mean x (1 +- 0.99 tol) and x (1 +- 1.01 tol)) under `bookkeeping_problems`; the stop within one window of
                 the float32 oracle's, as tests/test_hip_parity.py has it
An MI355X's figures are in profiles/train_update_error.json (`write_profile`)."""
import contextlib
import functools
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import nfisam_hip as nh
import test_train_gradient_cpu as G
import test_train_update_cpu as U
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR = 0.03
GRID = [(b, t) for b in U.BETAS for t in U.TS]
MAX_T = max(U.TS)


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


@contextlib.contextmanager
def switches(form):
    """NFISAM_* switches (without the prefix) for the launches inside; the environment is restored on exit."""
    old = {"NFISAM_" + k: os.environ.get("NFISAM_" + k) for k, _ in form}
    try:
        for k, v in form:
            os.environ["NFISAM_" + k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def form_name(form):
    return "default" if not form else ",".join("%s=%s" % kv for kv in form)


DEFAULT, UNFUSED, NO_IMAGE = (), (("FUSED_ADAM", "0"),), (("PAIR_IMAGE", "0"),)

# (name, [(n, D)], K, H, L): one TrainBatch each
Shape = namedtuple("Shape", "name cliques K H L")
SHAPES = [Shape("n96-d2k5h4l1", ((96, 2),), 5, 4, 1), Shape("n130-d5k9h8l1", ((130, 5),), 9, 8, 1), Shape("n64-d3k9h5l1", ((64, 3),), 9, 5, 1),
          Shape("n100-d3k5h16l2", ((100, 3),), 5, 16, 2), Shape("ragged", ((129, 3), (1, 5), (64, 2)), 9, 8, 1)]
TRAINED = "trained3"


def shape_of(name):
    if name == TRAINED:
        c = G.case(TRAINED)
        return Shape(TRAINED, ((c.n, c.D),), c.K, c.H, c.L)
    return [s for s in SHAPES if s.name == name][0]


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> [(blob, x) per clique], float32, read-only."""
    s = shape_of(name)
    if name == TRAINED:
        inp = G.inputs(TRAINED)
        return [(inp["blob"], inp["x"])]
    out = [G.make_problem(n, D, s.K, s.H, s.L, seed=8100 + 10 * SHAPES.index(s) + j) for j, (n, D) in enumerate(s.cliques)]
    for b, x in out:
        b.setflags(write=False)
        x.setflags(write=False)
    return out


def new_batch(name, max_iters, beta1=0.9, beta2=0.999, lr=LR, kps=None):
    s = shape_of(name)
    xs = [dev(x) for _, x in problem(name)]
    if kps is None:
        kps = [nh.pack(dev(b), D, s.K, s.H, s.L) for (b, _), (_, D) in zip(problem(name), s.cliques)]
    return nh.TrainBatch(xs, [k.clone() for k in kps], s.K, s.H, G.B, s.L, lr=lr, max_iters=max_iters, early_stop=False, beta1=beta1,
                         beta2=beta2)


def twin_gradient(name, kps=None, twin=None):
    """The gradient the Adam kernel consumes at the parameters `kps` (default: as packed): the first moment of one step() of a
    batch at beta1 = beta2 = 0 -> [g per clique, kernel layout, float32 numpy].  `twin`: a batch to reuse (it is reset)."""
    if twin is None:
        twin = new_batch(name, 1, beta1=0.0, beta2=0.0, kps=kps)
    else:
        twin.reset(kparams=kps)
    twin.step()
    torch.cuda.synchronize()
    assert twin.state()["step"] == 1 and twin.state()["domain_err"] == 0
    return [m.cpu().numpy().copy() for m in twin.m]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def seed_moments(g, beta1, t, seed):
    """Moments by the recipe of the CPU grid around a copy of g that is scaled down, per element and for every other element, by
    a log-uniform factor in [1e-6, 1]: there sqrt(v) comes near eps while g itself stays what the kernel computes."""
    rng = np.random.RandomState(seed)
    scale = np.ones(g.size)
    scale[1::2] = np.exp(rng.uniform(np.log(1e-6), 0.0, scale[1::2].size))
    return U.seeded_moments((g.astype(np.float64) * scale).astype(np.float32), beta1, t, seed + 1)


def set_state(tb, c, step, have_avg=0, loss_avg=0.0):
    words = np.zeros(tb.states.shape[1], dtype=np.int32)
    words[0], words[2] = step, have_avg
    words[3] = np.array([loss_avg], dtype=np.float32).view(np.int32)[0]
    tb.states[c].copy_(torch.from_numpy(words))


def padding(name):
    s = shape_of(name)
    return [np.tile(nh.layout_map(D, s.K, s.H) < 0, s.L) for _, D in s.cliques]


def worst(verdicts):
    out = dict(r_m=0.0, r_v=0.0, r_th=0.0, R32=0.0, quotient=0.0, problems=[])
    for v in verdicts:
        for k in ("r_m", "r_v", "r_th", "R32"):
            out[k] = max(out[k], v[k])
        out["quotient"] = max(out["quotient"], v["r_th"] / max(v["R32"], 1e-300))
        out["problems"] += v["problems"]
    out["bound"] = U.bound(out["R32"])
    return out


# ------------------------------------------------------------------ one step -------------
def measure_one_step(name, form):
    """Every (beta, t) of the grid on one reused TrainBatch (its cfg, parameters, moments and state rewritten before each step)
    -> (the worst figures, [what went wrong])."""
    s = shape_of(name)
    wrong, verdicts = [], []
    with switches(form):
        g = twin_gradient(name)
        g2 = twin_gradient(name)
        if not all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(g, g2)):
            wrong.append("two twins disagree")
        tb = new_batch(name, MAX_T + 1)
        kp0 = [k.clone() for k in tb.kparams]
        th0 = [k.cpu().numpy().copy() for k in kp0]
        pads = padding(name)
        for gi, (b, t) in enumerate(GRID):
            tb.cfg.beta1, tb.cfg.beta2, tb.cfg.max_iters = b[0], b[1], t + 1
            moments = [seed_moments(gc, b[0], t, 977 * gi + c) for c, gc in enumerate(g)]
            for c, (m0, v0) in enumerate(moments):
                tb.kparams[c].copy_(kp0[c])
                tb.m[c].copy_(torch.from_numpy(m0))
                tb.v[c].copy_(torch.from_numpy(v0))
                set_state(tb, c, t - 1)
            tb.step()
            torch.cuda.synchronize()
            cfg = U.adam_cfg(LR, *b)
            for c, (m0, v0) in enumerate(moments):
                st = tb.state(c)
                if st["step"] != t or st["stop"] != 0 or st["domain_err"] != 0:
                    wrong.append("state %s after the step at t = %d" % (st, t))
                m1, v1, th1 = (a[c].cpu().numpy() for a in (tb.m, tb.v, tb.kparams))
                v = U.adam_verdict(g[c], m0, v0, th0[c], m1, v1, th1, t, cfg)
                if v["problems"]:
                    wrong.append("%s beta %s t %d clique %d: %s" % (name, b, t, c, v["problems"]))
                p = pads[c]
                if np.any(m1[p] != 0) or np.any(v1[p] != 0) or np.any(th1[p] != 0):
                    wrong.append("padding moved at beta %s t %d" % (b, t))
                verdicts.append(v)
    rec = worst(verdicts)
    rec.update(case=name, what="one-step", form=form_name(form), steps=len(GRID))
    return rec, wrong


ONE_STEP = [(s.name, f) for s in SHAPES for f in (DEFAULT, UNFUSED) + ((NO_IMAGE,) if s.L > 1 else ())] + [(TRAINED, DEFAULT)]


def _show(rec):
    print("%-16s %-10s %-16s r_m %5.2f  r_v %5.2f  r_th %6.2f  R32 %5.2f  bound %5.1f  quotient %4.2f"
          % (rec["case"], rec["what"], rec["form"], rec["r_m"], rec["r_v"], rec["r_th"], rec["R32"], rec["bound"], rec["quotient"]))


@pytest.mark.parametrize("name,form", ONE_STEP, ids=["%s-%s" % (n, form_name(f)) for n, f in ONE_STEP])
def test_one_step_from_a_seeded_state_per_element(name, form):
    rec, wrong = measure_one_step(name, form)
    _show(rec)
    assert not wrong, wrong[:5]
    assert rec["r_m"] <= U.RM_MAX and rec["r_v"] <= U.RV_MAX and rec["R32"] <= U.R32_TH_MAX


# ------------------------------------------------------------------ a chain of steps -----
CHAIN_STEPS = 12
CHAINS = [(n, f, s0) for n in ("n96-d2k5h4l1", "n100-d3k5h16l2") for f in (DEFAULT, UNFUSED) for s0 in (0, 244, 122)]


def loss_reference(name, c, kparams):
    """The float64 NLL at the parameters `kparams` (kernel layout, device) with the scale and R32 of `G.loss_ratio`."""
    s = shape_of(name)
    (n, D), x = s.cliques[c], problem(name)[c][1]
    blob = nh.unpack(kparams, D, s.K, s.H, s.L).cpu().numpy()
    loss64, _, lp64 = CO.nll_grad(x, blob, s.K, s.H, G.B, s.L, dtype=np.float64)[:3]
    ref = dict(loss64=loss64, scale_loss=G.EPS32 * float(np.mean(np.abs(lp64))) * (G.loss_depth(n, D, s.L) + 2))
    ref["R32_loss"] = G.loss_ratio(CO.nll_grad(x, blob, s.K, s.H, G.B, s.L, dtype=np.float32)[0], ref)
    return ref


def measure_chain(name, form, s0):
    wrong, verdicts, loss_q = [], [], 0.0
    b = U.BETAS[0]
    cfg = U.adam_cfg(LR, *b)
    with switches(form):
        tb = new_batch(name, s0 + CHAIN_STEPS, *b)
        twin = new_batch(name, 1, beta1=0.0, beta2=0.0)
        if s0 > 0:
            m0, v0 = seed_moments(twin_gradient(name)[0], b[0], s0 + 1, 4242 + s0)
            tb.m[0].copy_(torch.from_numpy(m0))
            tb.v[0].copy_(torch.from_numpy(v0))
            set_state(tb, 0, s0)
        for k in range(CHAIN_STEPS):
            t = s0 + k + 1
            kp = tb.kparams[0].clone()
            th0, m0, v0 = (a[0].cpu().numpy().copy() for a in (tb.kparams, tb.m, tb.v))
            g = twin_gradient(name, [kp], twin)[0]
            tb.step()
            torch.cuda.synchronize()
            if tb.state()["step"] != t or tb.state()["stop"] != 0:
                wrong.append("state %s after call %d" % (tb.state(), k))
            m1, v1, th1 = (a[0].cpu().numpy() for a in (tb.m, tb.v, tb.kparams))
            v = U.adam_verdict(g, m0, v0, th0, m1, v1, th1, t, cfg)
            if v["problems"]:
                wrong.append("transition to t = %d: %s" % (t, v["problems"]))
            verdicts.append(v)
            ref = loss_reference(name, 0, kp)
            r = G.loss_ratio(float(tb.iter_loss[0][t - 1].item()), ref)
            loss_q = max(loss_q, r / G.bound(ref["R32_loss"]))
            if r > G.bound(ref["R32_loss"]):
                wrong.append("iter_loss[%d]: ratio %.3g, bound %.3g" % (t - 1, r, G.bound(ref["R32_loss"])))
        before = [a.cpu().numpy().copy() for a in (tb.kparams[0], tb.m[0], tb.v[0], tb.iter_loss[0], tb.states)]
        tb.step()                                                              # at step == max_iters: no bit may change
        torch.cuda.synchronize()
        after = [a.cpu().numpy() for a in (tb.kparams[0], tb.m[0], tb.v[0], tb.iter_loss[0], tb.states)]
        if not all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(before, after)):
            wrong.append("a call at step == max_iters changed something")
        il = after[3]
        if s0 > 0 and np.any(il[:s0] != 0):
            wrong.append("iter_loss written in front of the first step")
    rec = worst(verdicts)
    rec.update(case=name, what="chain@%d" % s0, form=form_name(form), steps=CHAIN_STEPS, loss_over_bound=loss_q)
    return rec, wrong


@pytest.mark.parametrize("name,form,s0", CHAINS, ids=["%s-%s-from%d" % (n, form_name(f), s) for n, f, s in CHAINS])
def test_a_chain_of_steps_every_transition_and_loss(name, form, s0):
    rec, wrong = measure_chain(name, form, s0)
    _show(rec)
    print("    loss ratio / bound: %.3f" % rec["loss_over_bound"])
    assert not wrong, wrong[:5]
    assert rec["r_m"] <= U.RM_MAX and rec["r_v"] <= U.RV_MAX and rec["R32"] <= U.R32_TH_MAX


# ------------------------------------------------------------------ whole runs -----------
RUN_FORMS = ["graph", "eager", "async"]
RUNS = [(rc, f) for rc in U.RUN_CASES for f in RUN_FORMS if f != "async" or rc[4] == 1]


def run_batch(problems, K, H, L, lr, cfg, form, state0=None):
    """One TrainBatch over [(blob, x)] under the window rule `cfg`, run in the given form -> ([iter_loss], [state]) or None when
    `launch_async` refuses the plan.  `state0` = (have_avg, loss_avg): preset state words of clique 0."""
    tb = nh.TrainBatch([dev(x) for _, x in problems], [nh.pack(dev(b), x.shape[1], K, H, L) for b, x in problems], K, H, G.B, L, lr=lr,
                       max_iters=cfg.max_iters, average_window=cfg.window, loss_delta_tol=cfg.tol)
    if state0 is not None:
        set_state(tb, 0, 0, *state0)
    if form == "async":
        if not tb.launch_async():
            return None
    else:
        done = tb.run(use_graph=form == "graph")
    torch.cuda.synchronize()
    states = [tb.state(c) for c in range(len(problems))]
    if form != "async":
        assert done == [s["step"] for s in states]
    assert all(s["domain_err"] == 0 for s in states)
    return [il.cpu().numpy() for il in tb.iter_loss], states


def measure_run(rc, form):
    n, D, K, H, L, wnd, tol, iters, lr, seed = rc
    cfg = U.Book(iters, wnd, tol)
    out = run_batch([U.run_problem(n, D, K, H, L, seed)], K, H, L, lr, cfg, form)
    if out is None:
        return None, None
    (il,), (st,) = out
    bad, gr = U.bookkeeping_problems(il, st, cfg)
    rec = dict(case=U.run_id(rc), what="run", form=form, step=st["step"], stop=st["stop"], oracle_step=U.oracle_run(rc)[1],
               undetermined=len(gr["undetermined"]), closest=float(gr["closest"]), loss_avg_error_over_bound=float(gr["avg_err_over_bound"]))
    return rec, bad


@pytest.mark.parametrize("rc,form", RUNS, ids=["%s-%s" % (U.run_id(rc), f) for rc, f in RUNS])
def test_whole_run_stops_where_the_float64_rule_demands(rc, form):
    rec, bad = measure_run(rc, form)
    if rec is None:
        pytest.skip("launch_async does not take this plan here")
    print(rec)
    assert not bad, bad
    assert abs(rec["step"] - rec["oracle_step"]) <= rc[5]                       # (tests/test_hip_parity.py's loose statement, unchanged)


@pytest.mark.parametrize("form", ["graph", "eager"])
def test_ragged_batch_every_clique_under_its_own_record(form):
    K, H, L = 9, 8, 1
    cfg = U.Book(500, 7, 3e-3)
    problems = [U.run_problem(64, 3, K, H, L, 6), U.run_problem(70, 1, K, H, L, 9), U.run_problem(96, 2, K, H, L, 5)]
    ils, states = run_batch(problems, K, H, L, 0.03, cfg, form)
    for il, st in zip(ils, states):
        bad, gr = U.bookkeeping_problems(il, st, cfg)
        print(st, gr["undetermined"], gr["closest"])
        assert not bad, bad


@pytest.mark.parametrize("form", ["graph", "eager", "async"])
def test_budget_that_ends_inside_a_window_takes_no_decision(form):
    n, D, K, H, L, wnd, _, _, lr, seed = U.RUN_CASES[0]
    cfg = U.Book(610, wnd, 0.0)                                                 # (tol = 0: delta < 0 never holds -- the run reaches the budget)
    out = run_batch([U.run_problem(n, D, K, H, L, seed)], K, H, L, lr, cfg, form)
    if out is None:
        pytest.skip("launch_async does not take this plan here")
    (il,), (st,) = out
    bad, gr = U.bookkeeping_problems(il, st, cfg)
    assert not bad, bad
    assert st["step"] == 610 and st["stop"] == 0 and gr["last_end"] == 600


EDGE_TOL = 5e-3      # 0.99 tol and 1.01 tol leave delta 2.5e-5 .. 7.6e-5 from tol: outside the band (asserted)


@pytest.mark.parametrize("form", ["graph", "eager"])
def test_seeded_rule_edges_one_chunk_from_a_preset_state(form):
    n, D, K, H, L, wnd, _, _, _, seed = U.RUN_CASES[0]
    cfg = U.Book(wnd, wnd, EDGE_TOL)
    prob = [U.run_problem(n, D, K, H, L, seed)]
    (il,), (st,) = run_batch(prob, K, H, L, 1e-12, cfg, form)                   # the first pass: the window mean (lr = 1e-12: the loss stands still)
    assert st == dict(st, step=wnd, stop=0, have_avg=1) and not U.bookkeeping_problems(il, st, cfg)[0]
    mean = np.float32(st["loss_avg"])
    # have_avg = 1 with loss_avg = 0.0: no stop, and the average is updated
    (il0,), (st0,) = run_batch(prob, K, H, L, 1e-12, cfg, form, state0=(1, 0.0))
    assert st0["stop"] == 0 and st0["step"] == wnd and st0["loss_avg"] == st["loss_avg"]
    assert not U.bookkeeping_problems(il0, st0, cfg, avg0=0.0)[0]
    for factor, stops in [(1 + 0.99 * EDGE_TOL, 1), (1 - 0.99 * EDGE_TOL, 1), (1 + 1.01 * EDGE_TOL, 0), (1 - 1.01 * EDGE_TOL, 0)]:
        avg0 = np.float32(float(mean) * factor)
        (il1,), (st1,) = run_batch(prob, K, H, L, 1e-12, cfg, form, state0=(1, float(avg0)))
        bad, gr = U.bookkeeping_problems(il1, st1, cfg, avg0=float(avg0))
        print("loss_avg = mean x %.5f: delta %.6f  stop %d" % (factor, gr["deltas"][wnd], st1["stop"]))
        assert not bad, bad
        assert gr["undetermined"] == [] and st1["stop"] == stops and st1["step"] == wnd


# ------------------------------------------------------------------ the profile ----------
def write_profile(path):
    """Every case x form -> the JSON of profiles/train_update_error.json.  From the repository root, on an MI355X:
        PYTHONPATH=nf-isam_amd:.:tests python tests/test_train_update_gpu.py profiles/train_update_error.json"""
    import json
    recs, problems = [], []
    for name, form in ONE_STEP:
        rec, wrong = measure_one_step(name, form)
        recs.append(rec)
        problems += wrong
    for name, form, s0 in CHAINS:
        rec, wrong = measure_chain(name, form, s0)
        recs.append(rec)
        problems += wrong
    runs = []
    for rc, form in RUNS:
        rec, bad = measure_run(rc, form)
        if rec is not None:
            runs.append(rec)
            problems += bad
    for r in recs:
        r.pop("problems")
    q = max(recs, key=lambda r: r["quotient"])

    def rnd(o):
        if isinstance(o, float):
            return float("%.4g" % o)
        if isinstance(o, list):
            return [rnd(v) for v in o]
        return {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else o
    out = {
        "what": "per-element error of the Adam update of TrainBatch.step() (one step from seeded states over the (beta, t) grid; chains of "
                "twelve steps) against torch.optim.Adam in float64, and the stop rule of whole runs replayed in float64 on the device's own "
                "loss record: tests/test_train_update_cpu.py (graders, cases), tests/test_train_update_gpu.py (this writer)",
        "ratio": "r_m = |m1 - m64| / (2^-24 (b1 |m0| + (1 - b1) |g|)), r_v = |v1 - v64| / (2^-24 v64), r_th = |th1 - (th0 - u)| / "
                 "(2^-24 (|th0| + |u|)), u from the device's own m1, v1; the largest over all elements and all steps of a record",
        "bound": "r_m, r_v <= 4; r_th <= 8 max(R32, 4) per step, R32 <= 16 (the float32 replay on the same inputs); loss_avg within "
                 "(wnd + 2) 2^-24 mean|l|; at most one undetermined window (|delta - tol| <= 2e-5) per run",
        "device": torch.cuda.get_device_name(0),
        "largest_device_over_oracle": {"quotient": q["quotient"], "case": q["case"], "what": q["what"], "form": q["form"]},
        "largest_device_ratio": {k: max(r[k] for r in recs) for k in ("r_m", "r_v", "r_th")},
        "largest_loss_ratio_over_bound": max(r["loss_over_bound"] for r in recs if "loss_over_bound" in r),
        "problems": problems,
        "records": recs,
        "runs": runs}
    with open(path, "w") as f:
        json.dump(rnd(out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    import sys
    write_profile(sys.argv[1])
