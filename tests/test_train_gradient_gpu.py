"""Every form of the training gradient graded per parameter against float64: the grader, the cases, the references and the bound
of tests/test_train_gradient_cpu.py (read its docstring first).

    max r <= 8 max(R32, 4) over EVERY parameter and EVERY dL/dx element; R32: the float32 oracle's ratio, R32 <= 32.

What is graded, one launch each:
  nh.backward, NLL mode with want_gx   kgrad / n, gx / n and the loss of every NLL case under NFISAM_TRAIN unset, wide and split;
                                       padding entries of the kernel layout exactly 0; the tails cases' init_param exactly 0
  nh.backward, VJP mode                the general cases (gz, gl = randn) and the knot cases (gl = 0), same three families
  the training launches themselves     TrainBatch(..., max_iters = 1, early_stop = False, beta1 = 0) and one step(): with beta1 = 0 the
                                       first moment tb.m[c] IS the gradient the Adam kernel consumed -- reduced over slabs or atomics
                                       by whichever path the form takes, the fused-Adam close included -- read through public state
                                       only.  (A form that refused beta1 = 0 would be run at 0.9, m / 0.1 graded with 2 2^-24 |g64|
                                       added to the scale: the rounding of the product and of the quotient.)  tb.m and tb.v at padding
                                       exactly 0.  Forms are CALL-time switches of nsf_knobs.h, flipped in-process and restored:
      L = 1, (5,9,8) and (12,9,8)      default, NFISAM_HALF=0, NFISAM_DIM_MAJOR=0, NFISAM_LEAN=0, NFISAM_FUSED_ADAM=0,
                                       NFISAM_TILES_PER_BLOCK=2, NFISAM_BIG_W=1 and 8
      L = 1, (5,16,8) (12,5,4) (20,9,16) (100,9,8)       default and NFISAM_DIM_MAJOR=0
      L > 1                            default, NFISAM_PAIR=0, =1, NFISAM_PAIR_STASH=0, NFISAM_PAIR_IMAGE=0, NFISAM_DIM_PAIRING=0
      ragged                           (n, D) = (130,5) (33,12) (65,1) (1,4) in ONE TrainBatch, L = 1 and 2, each clique against its own
                                       reference
      atomic sink                      129 tiles of 64 particles (NFISAM_TRAIN=wide) and of 32 (split) at D = 2, K = 5: past
                                       NFISAM_SLAB_MAX_TILES (read once per process; left alone)
Every test prints the device's ratio, R32 and their quotient; a training form's record says whether its bits equal the default
form's, i.e. whether the switch selected another kernel at that shape (launches that sum with float atomics -- the atomic sink,
nh.backward's single gradient copy -- have no fixed bits to compare).  An MI355X's figures are in profiles/train_gradient_error.json
(`write_profile`): no form exceeds the bound.  The largest parameter ratio at n >= 33 is 10.8 (VJP, L = 2, H = 4, wide family; oracle 8.4),
the largest device / oracle quotient there 3.1 (D = 1); the single particle at L = 2 reads 138 in every form (oracle 22.8, bound 182:
quotient 6.1).  dL/dx: at most 20.0 (the knot case at K = H = 16; oracle 7.4), quotient at most 4.4.  Loss: at most 0.5."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_train_gradient_cpu import (B, CASE_IDS, EPS32, R32_MAX, bound, case, gx_ratio, inputs, loss_ratio, param_ratio, ragged_names,
                                     reference)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILIES = ["auto", "wide", "split"]
NLL_CASES = [n for n in CASE_IDS if case(n).kind in ("nll", "trained", "tails")]
VJP_CASES = [n for n in CASE_IDS if case(n).kind in ("vjp", "knots")]


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)              # (a copy: the shared inputs are read-only)


@contextlib.contextmanager
def switches(env):
    """NFISAM_* switches (without the prefix) for the launches inside; every one of them must be unset outside."""
    names = ["NFISAM_" + k for k in env]
    assert not any(n in os.environ for n in names), names
    try:
        for n, v in zip(names, env.values()):
            os.environ[n] = v
        yield
    finally:
        for n in names:
            os.environ.pop(n, None)


def family_env(family):
    return {} if family == "auto" else {"TRAIN": family}


def padding(c):
    return torch.from_numpy(np.tile(nh.layout_map(c.D, c.K, c.H) < 0, c.L)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _record(name, what, form, ref, r, r_x=None, r_loss=None, same=None):
    c = case(name)
    rec = dict(case=name, what=what, form=form, n=c.n, D=c.D, K=c.K, H=c.H, L=c.L, R32=ref["R32"], device=float(r),
               quotient=float(r) / max(ref["R32"], 1e-300))
    if r_x is not None:
        rec.update(R32_x=ref["R32_x"], device_x=float(r_x), quotient_x=float(r_x) / max(ref["R32_x"], 1e-300))
    if r_loss is not None:
        rec.update(R32_loss=ref["R32_loss"], device_loss=float(r_loss))
    if same is not None:
        rec["bits_equal_default"] = bool(same)
    return rec


def _show(rec):
    s = "%-24s %-14s %-18s parameters: device %7.2f  R32 %6.2f  quotient %5.2f" % (rec["case"], rec["what"], rec["form"], rec["device"],
                                                                                     rec["R32"], rec["quotient"])
    if "device_x" in rec:
        s += "   dL/dx: %7.2f  %6.2f  %5.2f" % (rec["device_x"], rec["R32_x"], rec["quotient_x"])
    if "device_loss" in rec:
        s += "   loss: %5.2f  %5.2f" % (rec["device_loss"], rec["R32_loss"])
    if "bits_equal_default" in rec:
        s += "   bits == default: %s" % rec["bits_equal_default"]
    print(s)


def _assert_under_the_bound(rec):
    assert rec["R32"] <= R32_MAX
    assert rec["device"] <= bound(rec["R32"]), rec
    if "device_x" in rec:
        assert rec["R32_x"] <= R32_MAX
        assert rec["device_x"] <= bound(rec["R32_x"]), rec
    if "device_loss" in rec:
        assert rec["device_loss"] <= bound(rec["R32_loss"]), rec


# ------------------------------------------------------------------ nh.backward ----------
@functools.lru_cache(maxsize=None)
def device_backward(name, family):
    """One nh.backward launch of the case -> (kgrad [L Pk], g [L P] float64, gx [n, D] float64, loss or None), NLL mode: / n."""
    c, inp = case(name), inputs(name)
    kp = nh.pack(dev(inp["blob"]), c.D, c.K, c.H, c.L)
    nll = inp["gz"] is None
    with switches(family_env(family)):
        kg, gx, loss = nh.backward(dev(inp["x"]), kp, c.K, c.H, B, c.L, gz=None if nll else dev(inp["gz"]),
                                   gl=None if nll else dev(inp["gl"]), nll_mode=nll, want_gx=True)
        torch.cuda.synchronize()
    div = float(c.n) if nll else 1.0
    g = nh.unpack(kg, c.D, c.K, c.H, c.L).cpu().numpy().astype(np.float64) / div
    gx = gx.cpu().numpy().astype(np.float64) / div
    loss = float(loss.item()) / c.n + 0.5 * c.D * math.log(2 * math.pi) if nll else None
    return kg, g, gx, loss


def measure_backward(name, family):
    ref = reference(name)
    kg, g, gx, loss = device_backward(name, family)
    # (no bits-equal record here: nh.backward adds every tile into ONE gradient copy with float atomics, whose order is not fixed)
    return _record(name, "backward-nll" if loss is not None else "backward-vjp", family, ref, param_ratio(g, ref).max(),
                   gx_ratio(gx, ref).max(), None if loss is None else loss_ratio(loss, ref))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", NLL_CASES)
def test_backward_nll_gradient_dl_dx_and_loss_per_element(name, family):
    c, ref = case(name), reference(name)
    rec = measure_backward(name, family)
    _show(rec)
    kg, g, gx, loss = device_backward(name, family)
    assert float(kg[padding(c)].abs().max()) == 0.0                       # padding entries never receive gradient
    if c.kind == "tails":
        assert np.all(g[ref["where"][(0, 0, "init_param")]] == 0)           # no tolerance: every particle's dim 0 is the identity
    _assert_under_the_bound(rec)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", VJP_CASES)
def test_backward_vjp_gradient_and_dl_dx_per_element(name, family):
    c = case(name)
    rec = measure_backward(name, family)
    _show(rec)
    assert float(device_backward(name, family)[0][padding(c)].abs().max()) == 0.0
    _assert_under_the_bound(rec)


# ------------------------------------------------------------------ the training launches
DEFAULT = ()
L1_FORMS = [DEFAULT, (("HALF", "0"),), (("DIM_MAJOR", "0"),), (("LEAN", "0"),), (("FUSED_ADAM", "0"),), (("TILES_PER_BLOCK", "2"),),
            (("BIG_W", "1"),), (("BIG_W", "8"),)]
L1_TWO = [DEFAULT, (("DIM_MAJOR", "0"),)]
LN_FORMS = [DEFAULT, (("PAIR", "0"),), (("PAIR", "1"),), (("PAIR_STASH", "0"),), (("PAIR_IMAGE", "0"),), (("DIM_PAIRING", "0"),)]


def _nll(n, D, K, H, L):
    return "nll-n%d-d%dk%dh%dl%d" % (n, D, K, H, L)


TRAIN_STEPS = [((_nll(130, D, 9, 8, 1),), f) for D in (5, 12) for f in L1_FORMS]
TRAIN_STEPS += [((_nll(130, D, K, H, 1),), f) for D, K, H in [(5, 16, 8), (12, 5, 4), (20, 9, 16), (100, 9, 8)] for f in L1_TWO]
TRAIN_STEPS += [((_nll(n, D, 9, H, L),), f) for n, D, H, L in [(130, 7, 8, 3), (130, 12, 16, 2), (130, 6, 4, 2), (1, 4, 8, 2)] for f in LN_FORMS]
TRAIN_STEPS += [(tuple(ragged_names(L)), DEFAULT) for L in (1, 2)]
TRAIN_STEPS += [(("atomic64",), (("TRAIN", "wide"),)), (("atomic32",), (("TRAIN", "split"),))]


def form_name(form):
    return "default" if not form else ",".join("%s=%s" % kv for kv in form)


def step_id(names, form):
    return "%s-%s" % (names[0] if len(names) == 1 else "ragged-l%d" % case(names[0]).L, form_name(form))


@functools.lru_cache(maxsize=None)
def train_step(names, form):
    """One step() of ONE TrainBatch over the cases `names` (the same K, H, L) under the switches `form`, Adam's beta1 = 0
    -> [(m [L P] float32 in the torch layout, m at padding, v at padding, iter_loss[0], beta1) per clique]."""
    cs = [case(n) for n in names]
    K, H, L = cs[0].K, cs[0].H, cs[0].L
    assert all((c.K, c.H, c.L) == (K, H, L) for c in cs)
    with switches(dict(form)):
        xs = [dev(inputs(n)["x"]) for n in names]
        for beta1 in (0.0, 0.9):
            kps = [nh.pack(dev(inputs(n)["blob"]), c.D, K, H, L) for n, c in zip(names, cs)]
            tb = nh.TrainBatch(xs, kps, K, H, B, L, lr=1e-3, max_iters=1, early_stop=False, beta1=beta1)
            try:
                tb.step()
            except ValueError:
                if beta1 != 0.0:
                    raise
                continue
            break
        torch.cuda.synchronize()
        assert tb.state()["step"] == 1 and tb.state()["domain_err"] == 0
    out = []
    for j, c in enumerate(cs):
        pad = padding(c)
        out.append((nh.unpack(tb.m[j], c.D, K, H, L).cpu().numpy(), float(tb.m[j][pad].abs().max()), float(tb.v[j][pad].abs().max()),
                    float(tb.iter_loss[j][0].item()), beta1))
    return out


def measure_train_step(names, form):
    recs = []
    for j, name in enumerate(names):
        ref = reference(name)
        m, m_pad, v_pad, loss, beta1 = train_step(names, form)[j]
        g, extra = m.astype(np.float64), None
        if beta1 != 0.0:
            g, extra = g / (1.0 - beta1), 2 * EPS32 * np.abs(ref["g64"])
        same = None if form == DEFAULT else np.array_equal(_bits(m), _bits(train_step(names, DEFAULT)[j][0]))
        rec = _record(name, "train-step", form_name(form), ref, param_ratio(g, ref, extra).max(), None, loss_ratio(loss, ref), same)
        rec.update(m_padding=m_pad, v_padding=v_pad, beta1=beta1, cliques=len(names))
        recs.append(rec)
    return recs


@pytest.mark.parametrize("names,form", TRAIN_STEPS, ids=[step_id(*t) for t in TRAIN_STEPS])
def test_train_step_first_moment_is_the_gradient_per_parameter(names, form):
    for rec in measure_train_step(names, form):
        _show(rec)
        assert rec["m_padding"] == 0.0 and rec["v_padding"] == 0.0
        _assert_under_the_bound(rec)


def write_profile(path):
    """Every case x form -> the JSON of profiles/train_gradient_error.json.  From the repository root, on an MI355X:
        PYTHONPATH=nf-isam_amd:. python tests/test_train_gradient_gpu.py profiles/train_gradient_error.json"""
    import json
    recs = [measure_backward(n, f) for n in NLL_CASES + VJP_CASES for f in FAMILIES]
    recs += [r for names, form in TRAIN_STEPS for r in measure_train_step(names, form)]
    quot = [(r["quotient"], r["case"], r["what"], r["form"], "parameters") for r in recs]
    quot += [(r["quotient_x"], r["case"], r["what"], r["form"], "dL/dx") for r in recs if "quotient_x" in r]
    q = max(quot)

    def rnd(o):
        if isinstance(o, float):
            return round(o, 3)
        if isinstance(o, list):
            return [rnd(v) for v in o]
        return {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else o
    out = {
        "what": "per-element error of the training gradient (nh.backward in NLL and VJP mode; the first moment of one TrainBatch.step() "
                "at beta1 = 0) and of the float32 oracle (host) against the float64 oracle: tests/test_train_gradient_cpu.py (grader, "
                "cases), tests/test_train_gradient_gpu.py (this writer)",
        "ratio": "r_j = |g_j - g64_j| / (2^-24 (S_j + T_j) + sigma_j); dL/dx and loss as the grader's docstring has them; the largest "
                 "over all elements of a case",
        "bound": "device <= 8 max(R32, 4), R32 <= %g (R32: the float32 oracle's ratio on the same inputs)" % R32_MAX,
        "device": torch.cuda.get_device_name(0),
        "largest_device_over_oracle": {"quotient": q[0], "case": q[1], "what": q[2], "form": q[3], "of": q[4]},
        "largest_device_ratio": {"parameters": max(r["device"] for r in recs), "dL/dx": max(r["device_x"] for r in recs if "device_x" in r),
                                 "loss": max(r["device_loss"] for r in recs if "device_loss" in r)},
        "bits_equal_default": "whether the form's gradient has the default form's bits at that shape (false: the switch selected "
                              "another kernel or another summation order)",
        "records": recs}
    with open(path, "w") as f:
        json.dump(rnd(out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    import sys
    write_profile(sys.argv[1])
