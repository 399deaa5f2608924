"""Every posterior draw of nfisam_nsf_inverse and nfisam_nsf_posterior_walk graded by its backward error in float64: the grader,
the cases, the latent draws and the bound of tests/test_sampler_backward_cpu.py (read its docstring first).

    max r_z <= 8 max(R32, 4)   and   max r_ld <= 8 max(R32_ld, 4)    over EVERY element; R32: the float32 oracle's, R32 <= 64.

Kernels: nsf_inverse_kernel (every case of INVERSE_CASES: D = 1 .. 20, K = 2 .. 16, H = 4, 8, 16, L = 1 .. 3, given columns, a
marginal evaluation through the layer stride, fused normalisation with a drawn and a given angle column), and the walk in each
of its forms on its own: nsf_posterior_walk2_kernel (the default for L = 1, H = 8 / 16 while its LDS fits), nsf_posterior_walk_kernel
(NFISAM_WALK=plain, L = 2, H = 4, max_D = 20 at H = 16) and one nfisam_nsf_inverse call per clique with model_D.

Tolerance-free, with mean == NULL: a draw with |z| > B or NaN comes back with the bits of z and adds 0 to the log-det, everything
else is finite and |x| <= B.  In every form a particle's bits do not depend on n or on its place in the tile (each particle's
arithmetic is its own lane's, or lane pair's in the two-lane walk): n = 1, 64, 65, 130 and the last particle alone.

The ratios are printed per case; those of an MI355X are in profiles/sampler_backward_error.json: the largest r_z is 15.9
(L = 3, D = 7; the float32 oracle's 4.5, the largest device / oracle quotient, 3.6), the largest r_ld 7.0 (oracle 5.6), the walk's
4.8 (two-lane form, one clique of 19 dims; oracle 3.3).  The box property failed before the inverse spline clamped its result:
z = B came back as 5.00000048 (K = 2, dim 0)."""
import os

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sampler_backward_cpu import (B, CASE_IDS, INVERSE_CASES, N, R32_MAX, WALK_TREES, bound, case_norm, exact_failures, fixture,
                                       grade, grade_walk, reference, walk2_lds_bytes, walk_reference, walk_tree)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def kpack(blob, D, K, H, L):
    return nh.pack(torch.from_numpy(np.ascontiguousarray(blob)).to(DEV), D, K, H, L)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def device_inverse(c, z, given, rows=slice(None)):
    """-> (drawn [n, F], ld [n]) of the rows `rows`, through the whole model's parameters (model_D > D: the layer stride)."""
    kp = kpack(fixture()["blob_" + c.blob], c.model_D, c.K, c.H, c.L)
    kw = {}
    norm = case_norm(c)
    if norm is not None:
        kw = dict(mean=dev(norm[0]), std=dev(norm[1]), circular=torch.from_numpy(norm[2].astype(np.uint8)).to(DEV))
    x, ld = nh.inverse(dev(z[rows]), dev(given[rows]) if c.Ds else None, kp, c.K, c.H, B, c.L, want_logdet=True,
                       model_D=c.model_D, **kw)
    return x.cpu().numpy(), ld.cpu().numpy()


def measure_inverse(name):
    c, ref = INVERSE_CASES[CASE_IDS.index(name)], reference(name)
    x, ld = device_inverse(c, ref["z"], ref["given"])
    row = np.concatenate([ref["given"], x], 1) if c.Ds else x
    r_z, r_ld = grade(c, row, ref["z"], ld)
    return dict(case=name, D=c.D, Ds=c.Ds, K=c.K, H=c.H, L=c.L, model_D=c.model_D, normed=c.norm, R32_z=ref["R32_z"],
                R32_ld=ref["R32_ld"], device_r_z=float(r_z.max()), device_r_ld=float(r_ld.max())), x, ld


@pytest.mark.parametrize("name", CASE_IDS)
def test_inverse_draws_and_log_det_by_backward_error(name):
    c, ref = INVERSE_CASES[CASE_IDS.index(name)], reference(name)
    m, x, ld = measure_inverse(name)
    print("%-24s r_z: device %7.2f  float32 oracle %6.2f   r_ld: device %7.2f  float32 oracle %6.2f"
          % (name, m["device_r_z"], m["R32_z"], m["device_r_ld"], m["R32_ld"]))
    assert m["R32_z"] <= R32_MAX and m["R32_ld"] <= R32_MAX                     # the condition on the inputs
    assert np.all(np.isfinite(ld))
    if c.norm:
        assert np.all(np.isfinite(x[~np.isnan(ref["z"])]))
    else:
        assert not exact_failures(x, ref["z"], ld), exact_failures(x, ref["z"], ld)
    assert m["device_r_z"] <= bound(m["R32_z"]), m
    assert m["device_r_ld"] <= bound(m["R32_ld"]), m
    # a particle's bits depend neither on n nor on its place in the tile
    for rows in (slice(0, 1), slice(0, 64), slice(0, 65), slice(N - 1, N)):
        xs, lds = device_inverse(c, ref["z"], ref["given"], rows)
        assert np.array_equal(_bits(xs), _bits(x[rows])) and np.array_equal(_bits(lds), _bits(ld[rows])), (name, rows)


# ------------------------------------------------------------------ the walk -------------
def _entries(name):
    K, H, L, total, cliques = walk_tree(name)
    return [dict(kparams=kpack(q.blob, q.D_model, K, H, L), mean=dev(q.mean), std=dev(q.std),
                 circular=torch.from_numpy(q.circ.astype(np.uint8)).to(DEV), D_model=q.D_model, obs=q.obs, sep_cols=q.sep,
                 front_cols=q.front) for q in cliques]


def expected_form(name):
    """What `unit_walk` launches by default: the two-lane walk for L = 1 and H = 8 / 16 while its LDS is at most 150 KB."""
    K, H, L, total, cliques = walk_tree(name)
    max_D = max(q.D_model for q in cliques)
    fits = walk2_lds_bytes(max_D, K, H, L, nh.kparam_count) <= 150 * 1024
    return "two-lane" if (L == 1 and H % 8 == 0 and fits and max_D <= 64) else "plain"


def device_walk(name, Zt, form, entries=None, n=N, first=0):
    K, H, L, total, cliques = walk_tree(name)
    entries = entries or _entries(name)
    Z = dev(Zt[:, first:first + n])
    if form == "per-clique":                     # one nfisam_nsf_inverse call per clique (what FlowsPriorFactor.sample uses)
        S = torch.zeros(n, total, device=DEV)
        zrow = 0
        for q, e in zip(cliques, entries):
            given = ([dev(np.tile(q.obs, (n, 1)))] if len(q.obs) else []) + ([S[:, q.sep]] if q.sep else [])
            xs = torch.cat(given, 1).contiguous() if given else None
            F = len(q.front)
            S[:, q.front] = nh.inverse(Z[zrow:zrow + F].t().contiguous(), xs, e["kparams"], K, H, B, L, mean=e["mean"],
                                       std=e["std"], circular=e["circular"], model_D=q.D_model)
            zrow += F
        return S.cpu().numpy()
    assert "NFISAM_WALK" not in os.environ
    if form == "plain":
        os.environ["NFISAM_WALK"] = "plain"
    try:
        return nh.posterior_walk(entries, total, n, K, H, B, L, DEV, Zt=Z).cpu().numpy()
    finally:
        os.environ.pop("NFISAM_WALK", None)


def measure_walk(name, form, entries=None):
    ref = walk_reference(name)
    S = device_walk(name, ref["Zt"], form, entries)
    ran = expected_form(name) if form == "default" else form
    return dict(tree=name, form=form, kernel=ran, R32_z=ref["R32"], device_r_z=grade_walk(name, S, ref["Zt"])), S


@pytest.mark.parametrize("form", ["default", "plain", "per-clique"])
@pytest.mark.parametrize("name", WALK_TREES)
def test_walk_draws_by_backward_error_each_form_on_its_own(name, form):
    ref = walk_reference(name)
    entries = _entries(name)
    m, S = measure_walk(name, form, entries)
    print("%-14s %-10s (%s)  r_z per clique: device %s   float32 oracle %s"
          % (name, form, m["kernel"], " ".join("%6.2f" % r for r in m["device_r_z"]), " ".join("%5.2f" % r for r in m["R32_z"])))
    assert max(m["R32_z"]) <= R32_MAX
    assert np.all(np.isfinite(S))
    for r, r32 in zip(m["device_r_z"], m["R32_z"]):
        assert r <= bound(r32), m
    for n, first in ((1, 0), (64, 0), (65, 0), (1, N - 1)):
        Sn = device_walk(name, ref["Zt"], form, entries, n=n, first=first)
        assert np.array_equal(_bits(Sn), _bits(S[first:first + n])), (name, form, n, first)


def test_single_clique_trees_sit_on_either_side_of_the_lds_switch():
    assert expected_form("single-d19h16") == "two-lane" and expected_form("single-d20h16") == "plain"
    assert [expected_form(t) for t in WALK_TREES[:4]] == ["two-lane", "two-lane", "plain", "plain"]


@pytest.mark.parametrize("name", WALK_TREES)
def test_the_default_form_is_the_kernel_the_lds_rule_names(name):
    """`expected_form` restates the rule of `unit_walk`; the launch itself shows which kernel ran: the two kernels round differently
    somewhere, so the default form's bits are the plain walk's exactly where the rule names the plain walk."""
    ref = walk_reference(name)
    entries = _entries(name)
    same = np.array_equal(_bits(device_walk(name, ref["Zt"], "default", entries)), _bits(device_walk(name, ref["Zt"], "plain", entries)))
    assert same == (expected_form(name) == "plain"), (name, same)


def write_profile(path):
    """Every case's ratios -> the JSON of profiles/sampler_backward_error.json.  From the repository root, on an MI355X:
        PYTHONPATH=nf-isam_amd:. python tests/test_sampler_backward_gpu.py profiles/sampler_backward_error.json"""
    import json
    inv = [measure_inverse(name)[0] for name in CASE_IDS]
    walk = [measure_walk(name, form)[0] for name in WALK_TREES for form in ("default", "plain", "per-clique")]
    quot = [(m["device_r_z"] / m["R32_z"], m["case"], "r_z") for m in inv] + [(m["device_r_ld"] / m["R32_ld"], m["case"], "r_ld") for m in inv]
    quot += [(a / b, "%s / %s / clique %d" % (m["tree"], m["form"], j), "r_z") for m in walk
             for j, (a, b) in enumerate(zip(m["device_r_z"], m["R32_z"]))]
    q = max(quot)

    def rnd(o):
        if isinstance(o, float):
            return round(o, 3)
        if isinstance(o, list):
            return [rnd(v) for v in o]
        return {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else o
    out = {
        "what": "backward error of every posterior draw of nfisam_nsf_inverse and nfisam_nsf_posterior_walk and of the float32 oracle "
                "(host), in float64: tests/test_sampler_backward_cpu.py (grader, cases), tests/test_sampler_backward_gpu.py (this writer)",
        "ratio": "r_z = |fwd64(x) - z| / (2^-24 L ((B + |z|) + slope (B + |x|))), r_ld = |ld + sum lad64| / (2^-24 L sum (1 + "
                 "|d lad/dx| (B + |x|))); the largest over all elements of a case (n = %d, B = %g)" % (N, B),
        "bound": "device <= 8 max(R32, 4), R32 <= %g (R32: the float32 oracle's ratio on the same inputs)" % R32_MAX,
        "device": torch.cuda.get_device_name(0),
        "largest_device_over_oracle": {"quotient": q[0], "case": q[1], "ratio": q[2]},
        "largest_device_ratio": {"inverse_r_z": max(m["device_r_z"] for m in inv), "inverse_r_ld": max(m["device_r_ld"] for m in inv),
                                 "walk_r_z": max(max(m["device_r_z"]) for m in walk)},
        "walk_kernel": "`kernel`: the form unit_walk launches for the tree (two-lane: nsf_posterior_walk2_kernel; plain: "
                       "nsf_posterior_walk_kernel; per-clique: one nfisam_nsf_inverse call per clique), by the LDS rule and confirmed by "
                       "test_the_default_form_is_the_kernel_the_lds_rule_names; ratios per clique in walk order",
        "inverse": inv, "walk": walk}
    with open(path, "w") as f:
        json.dump(rnd(out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    import sys
    write_profile(sys.argv[1])
