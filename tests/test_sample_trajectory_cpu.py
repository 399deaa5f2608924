"""The trajectory-error evaluator without a GPU: the float64 oracle of tests/test_sample_trajectory_gpu.py and what pins it
(numpy's SVD route, the reference's own `kabsch_umeyama` outputs in tests/golden/trajectory_error.npz, mpmath at 60 digits on
ill-conditioned cases), `utils.Functions.kabsch_umeyama`, the tables and every refusal that needs no device, the surface of
the new C entries, and `NFiSAM.posterior_trajectory_error`'s errors before anything is launched.

The oracle (`oracle_trajectory`, `oracle_rpe`) evaluates the formulas of include/nfisam_hip.h on the float32 points cast to
float64: elementwise parts in numpy float64, EVERY sum by math.fsum, which rounds the exact sum once -- so a comparison with
the device bounds the device's error (the oracle's own few roundings per term are counted in the bounds of `bounds`).

`trajectory_case`, `bounds` and `mp_trajectory` are shared with the GPU tests."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from utils import Functions as FN
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -53


def wrap_pi(t):
    return (t + np.pi) % (2.0 * np.pi) - np.pi


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def oracle_trajectory(x, entries, mode="rigid", reflect=False):
    """Per sample (row of x): theta, scale, t [n, 2], reflected, sse_traj, sse_landmark, sse_heading, resid [n, P] (|r_e|),
    and what the bounds are stated through: g, saa = sum |a'|^2, sbb = sum |b'|^2, kappa = g / sqrt(saa sbb) (1 where g = 0 or
    nothing is aligned), bbar [n, 2], lever = max_e |b_e - b_bar|, M = the largest coordinate met."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, P = x.shape[0], entries.size
    al = (entries["flags"] & nh.TRAJ_ALIGNED) != 0
    land = (entries["flags"] & nh.TRAJ_LANDMARK) != 0
    head = entries["col_th"] >= 0
    ax, ay, ath = entries["ax"], entries["ay"], entries["ath"]
    N = int(al.sum())
    out = dict(theta=np.zeros(n), scale=np.ones(n), t=np.zeros((n, 2)), reflected=np.zeros(n, dtype=bool), sse_traj=np.zeros(n),
               sse_landmark=np.zeros(n), sse_heading=np.zeros(n), resid=np.zeros((n, P)), g=np.zeros(n), saa=np.zeros(n),
               sbb=np.zeros(n), kappa=np.ones(n), bbar=np.zeros((n, 2)), lever=np.zeros(n), M=np.zeros(n))
    abar = (math.fsum(ax[al]) / N, math.fsum(ay[al]) / N) if N else (0.0, 0.0)
    for i in range(n):
        bx, by = x[i, entries["col_x"]], x[i, entries["col_y"]]
        theta, c, tx, ty, flip, bbar = 0.0, 1.0, 0.0, 0.0, 1.0, (0.0, 0.0)
        if N:
            bbar = (math.fsum(bx[al]) / N, math.fsum(by[al]) / N)
        if mode != "none":
            apx, apy, bpx, bpy = ax[al] - abar[0], ay[al] - abar[1], bx[al] - bbar[0], by[al] - bbar[1]
            dot, crs = math.fsum(list(apx * bpx) + list(apy * bpy)), math.fsum(list(apy * bpx) + list(-apx * bpy))
            dotm, crsm = math.fsum(list(apx * bpx) + list(-apy * bpy)), math.fsum(list(apx * bpy) + list(apy * bpx))
            saa, sbb = math.fsum(list(apx * apx) + list(apy * apy)), math.fsum(list(bpx * bpx) + list(bpy * bpy))
            g = math.hypot(dot, crs)
            if reflect and math.hypot(dotm, crsm) > g:
                g, dot, crs, flip = math.hypot(dotm, crsm), dotm, crsm, -1.0
            theta = 0.0 if g == 0.0 else math.atan2(crs, dot)
            if mode == "similarity":
                c = 1.0 if sbb == 0.0 else g / sbb
            cs, sn = math.cos(theta), math.sin(theta)
            tx = abar[0] - c * (cs * bbar[0] - sn * flip * bbar[1])
            ty = abar[1] - c * (sn * bbar[0] + cs * flip * bbar[1])
            out["g"][i], out["saa"][i], out["sbb"][i] = g, saa, sbb
            if g > 0.0:
                out["kappa"][i] = g / math.sqrt(saa * sbb)
        cs, sn = math.cos(theta), math.sin(theta)
        px, py = c * (cs * bx - sn * flip * by) + tx, c * (sn * bx + cs * flip * by) + ty
        r2 = (ax - px) ** 2 + (ay - py) ** 2
        bth = x[i, np.where(head, entries["col_th"], 0)]
        h = wrap_pi(np.where(flip < 0, theta - bth, bth + theta) - ath)
        out["theta"][i], out["scale"][i], out["t"][i], out["reflected"][i] = theta, c, (tx, ty), flip < 0
        out["sse_traj"][i], out["sse_landmark"][i] = math.fsum(r2[~land]), math.fsum(r2[land])
        out["sse_heading"][i] = math.fsum((h * h)[head])
        out["resid"][i] = np.sqrt(r2)
        out["bbar"][i] = bbar
        out["lever"][i] = np.sqrt((bx - bbar[0]) ** 2 + (by - bbar[1]) ** 2).max()
        out["M"][i] = max(np.abs(bx).max(), np.abs(by).max(), np.abs(ax).max(), np.abs(ay).max(), np.abs(px).max(), np.abs(py).max())
    return out


def _relative(px, py, th, i, j):
    cs, sn = np.cos(th[i]), np.sin(th[i])
    ex, ey = px[j] - px[i], py[j] - py[i]
    return cs * ex + sn * ey, cs * ey - sn * ex, wrap_pi(th[j] - th[i])


def oracle_rpe(x, entries, pairs, n_slots):
    """(trans [n_slots, n], rot [n_slots, n], D [n_slots, n]: the largest |d| met, for the bound)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    trans, rot, D = np.zeros((n_slots, n)), np.zeros((n_slots, n)), np.zeros((n_slots, n))
    fx, fy, fth = _relative(entries["ax"], entries["ay"], entries["ath"], pairs["i"], pairs["j"])
    for i in range(n):
        ex, ey, eth = _relative(x[i, entries["col_x"]], x[i, entries["col_y"]], x[i, np.maximum(entries["col_th"], 0)],
                                pairs["i"], pairs["j"])
        d2, r2 = (ex - fx) ** 2 + (ey - fy) ** 2, wrap_pi(eth - fth) ** 2
        for s in range(n_slots):
            m = pairs["slot"] == s
            trans[s, i], rot[s, i] = math.fsum(d2[m]), math.fsum(r2[m])
            D[s, i] = max(np.hypot(ex[m], ey[m]).max(), np.hypot(fx[m], fy[m]).max())
    return trans, rot, D


def bounds(o, entries, n=1):
    """The bounds the device results are held to, per sample, from operation counts and sum depths (the derivation is the
    docstring of tests/test_sample_trajectory_gpu.py).  `o` is `oracle_trajectory`'s dict.  -> dict of arrays."""
    P, N = entries.size, int(((entries["flags"] & nh.TRAJ_ALIGNED) != 0).sum())
    kN, kP = -(-N // 4) + 3, -(-P // 4) + 3
    aligned = o["g"] > 0.0
    e_rot = np.where(aligned, (math.sqrt(2.0) * (kN + 6) / o["kappa"] + 8.0) * U, 0.0)
    a_abs = 2.0 * (24 + kN) * U * (1.0 + o["scale"]) * o["M"]
    resid = a_abs + o["scale"] * o["lever"] * 2.0 * e_rot
    rel = 2.0 * kP * U
    return dict(e_rot=e_rot, a_abs=a_abs, resid=resid, rel=rel, theta=e_rot + 4 * U * np.pi, scale=o["scale"] * (e_rot + 4 * U),
                t=a_abs + o["scale"] * np.hypot(o["bbar"][:, 0], o["bbar"][:, 1]) * 2.0 * e_rot,
                heading=e_rot + 16 * U * np.pi)


def mp_trajectory(row, entries, mode="rigid", reflect=False, dps=60):
    """One sample at `dps` digits with mpmath: (theta, scale, (tx, ty), ate, heading_rms, landmark_rmse, kappa) as floats."""
    import mpmath as mp
    with mp.workdps(dps):
        f = lambda v: mp.mpf(float(v))                                            # noqa: E731  (exact: a double is a rational)
        al = (entries["flags"] & nh.TRAJ_ALIGNED) != 0
        land = (entries["flags"] & nh.TRAJ_LANDMARK) != 0
        a = [(f(e["ax"]), f(e["ay"]), f(e["ath"])) for e in entries]
        b = [(f(np.float32(row[e["col_x"]])), f(np.float32(row[e["col_y"]])),
              f(np.float32(row[e["col_th"]])) if e["col_th"] >= 0 else None) for e in entries]
        idx = [k for k in range(entries.size) if al[k]]
        N = len(idx)
        theta, c, tx, ty, flip, kappa = mp.mpf(0), mp.mpf(1), mp.mpf(0), mp.mpf(0), 1, mp.mpf(1)
        if mode != "none":
            abar = (mp.fsum(a[k][0] for k in idx) / N, mp.fsum(a[k][1] for k in idx) / N)
            bbar = (mp.fsum(b[k][0] for k in idx) / N, mp.fsum(b[k][1] for k in idx) / N)
            ap = [(a[k][0] - abar[0], a[k][1] - abar[1]) for k in idx]
            bp = [(b[k][0] - bbar[0], b[k][1] - bbar[1]) for k in idx]
            dot = mp.fsum(p[0] * q[0] + p[1] * q[1] for p, q in zip(ap, bp))
            crs = mp.fsum(p[1] * q[0] - p[0] * q[1] for p, q in zip(ap, bp))
            dotm = mp.fsum(p[0] * q[0] - p[1] * q[1] for p, q in zip(ap, bp))
            crsm = mp.fsum(p[0] * q[1] + p[1] * q[0] for p, q in zip(ap, bp))
            saa, sbb = mp.fsum(p[0] ** 2 + p[1] ** 2 for p in ap), mp.fsum(q[0] ** 2 + q[1] ** 2 for q in bp)
            g = mp.hypot(dot, crs)
            if reflect and mp.hypot(dotm, crsm) > g:
                g, dot, crs, flip = mp.hypot(dotm, crsm), dotm, crsm, -1
            theta = mp.mpf(0) if g == 0 else mp.atan2(crs, dot)
            if mode == "similarity" and sbb != 0:
                c = g / sbb
            if g != 0:
                kappa = g / mp.sqrt(saa * sbb)
            tx = abar[0] - c * (mp.cos(theta) * bbar[0] - mp.sin(theta) * flip * bbar[1])
            ty = abar[1] - c * (mp.sin(theta) * bbar[0] + mp.cos(theta) * flip * bbar[1])
        cs, sn = mp.cos(theta), mp.sin(theta)
        sse_t = sse_l = sse_h = mp.mpf(0)
        nt = nl = nh_ = 0
        for k in range(entries.size):
            px = c * (cs * b[k][0] - sn * flip * b[k][1]) + tx
            py = c * (sn * b[k][0] + cs * flip * b[k][1]) + ty
            r2 = (a[k][0] - px) ** 2 + (a[k][1] - py) ** 2
            if land[k]:
                sse_l, nl = sse_l + r2, nl + 1
            else:
                sse_t, nt = sse_t + r2, nt + 1
            if b[k][2] is not None:
                h = (theta - b[k][2] if flip < 0 else b[k][2] + theta) - a[k][2]
                h = h - 2 * mp.pi * mp.floor((h + mp.pi) / (2 * mp.pi))
                sse_h, nh_ = sse_h + h * h, nh_ + 1
        root = lambda s, m: float(mp.sqrt(s / m)) if m else float("nan")        # noqa: E731
        return float(theta), float(c), (float(tx), float(ty)), root(sse_t, nt), root(sse_h, nh_), root(sse_l, nl), float(kappa)


# ---- the data of the GPU tests --------------------------------------------------------------------------------------------------
SPECIAL = dict(exact=1, truth=2, mirrored=3, coincident=5)
N_MAX = 257


def trajectory_case(P, n=N_MAX, seed=20241021):
    """(x float32 [n, 3 P], entries): P entries at 100 m offsets with centimetre errors.  The first P - L are poses (columns
    3 e .. 3 e + 2, aligned, headings massed on both sides of +-pi), the last L = P // 5 (one from P = 3 on) landmarks outside
    the alignment.  The truth lies on multiples of 1/4 within [50, 150] and its headings are float32 values, so the special
    samples are EXACT in float32: sample 1 is the truth under theta = pi / 2, c = 2, t = (-30, 20) undone; sample 2 is the truth;
    sample 3 the truth mirrored (y -> 200 - y); sample 5 has every point at (120.5, 80.25).  Every other sample is the truth
    under its own rigid transform about the centre, undone, plus 1 cm noise."""
    rng = np.random.RandomState(seed + P)
    L = 0 if P < 3 else max(1, P // 5)
    walk = np.cumsum(rng.standard_normal((P, 2)), axis=0)
    walk = (walk - walk.mean(0)) / max(np.abs(walk - walk.mean(0)).max(), 1.0)
    a = np.round((100.0 + 45.0 * walk) * 4.0) / 4.0
    ath = wrap_pi(np.pi + 0.2 * rng.standard_normal(P)).astype(np.float32).astype(np.float64)
    x = np.zeros((n, 3 * P))
    centre = np.array([100.0, 100.0])
    for i in range(n):
        th = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        b = (a - centre) @ R + centre + rng.uniform(-5, 5, 2) + 0.01 * rng.standard_normal((P, 2))   # R(-th) (a - centre) + ...
        bth = wrap_pi(ath - th + 0.05 * rng.standard_normal(P))
        if i == SPECIAL["exact"]:                                  # a = 2 R(pi/2) b + t  <=>  b = R(-pi/2) (a - t) / 2
            d = a - np.array([-30.0, 20.0])
            b, bth = np.stack([d[:, 1], -d[:, 0]], axis=1) / 2.0, wrap_pi(ath - np.pi / 2)
        elif i == SPECIAL["truth"]:
            b, bth = a.copy(), ath.copy()
        elif i == SPECIAL["mirrored"]:
            b, bth = np.stack([a[:, 0], 200.0 - a[:, 1]], axis=1), wrap_pi(-ath)
        elif i == SPECIAL["coincident"]:
            b = np.tile([120.5, 80.25], (P, 1))
        x[i, 0::3], x[i, 1::3], x[i, 2::3] = b[:, 0], b[:, 1], bth
    x = x.astype(np.float32)
    cols = 3 * np.arange(P)
    entries = nh.pack_traj_entries(cols, cols + 1, np.where(np.arange(P) < P - L, cols + 2, -1), a, ath, landmark=np.arange(P) >= P - L)
    return x, entries


# ---- the oracle itself ------------------------------------------------------------------------------------------------------------
def _svd_fit(A, B):
    """numpy's SVD route with S = diag(1, d): (R, least-squares scale tr(D S) n / sum |b'|^2, d)."""
    da, db = A - A.mean(0), B - B.mean(0)
    Um, D, Vt = np.linalg.svd(da.T @ db / len(A))
    d = np.sign(np.linalg.det(Um) * np.linalg.det(Vt))
    S = np.array([1.0, d])
    return (Um * S) @ Vt, float(np.sum(D * S) * len(A) / np.sum(db * db)), d


@pytest.mark.parametrize("P", [2, 3, 40])
def test_oracle_equals_the_svd_route(P):
    x, entries = trajectory_case(P, n=12)
    al = (entries["flags"] & nh.TRAJ_ALIGNED) != 0
    A = np.stack([entries["ax"], entries["ay"]], axis=1)[al]
    for mode in ("rigid", "similarity"):
        o = oracle_trajectory(x, entries, mode)
        for i in range(x.shape[0]):
            if i == SPECIAL["coincident"]:
                assert o["theta"][i] == 0.0 and o["scale"][i] == 1.0 and o["g"][i] == 0.0
                continue
            B = x[i].astype(np.float64).reshape(-1, 3)[al][:, :2]
            R, c_ls, d = _svd_fit(A, B)
            tol = 1e-13 / max(o["kappa"][i], 1e-3)
            cs, sn = math.cos(o["theta"][i]), math.sin(o["theta"][i])
            assert np.abs(R - np.array([[cs, -sn], [sn, cs]])).max() <= tol, (P, mode, i)
            if i == SPECIAL["mirrored"] and al.sum() > 2:          # (two points are rank one: the sign of det is noise)
                assert d == -1.0                                   # reflect off: the proper fit of a mirrored set
            if mode == "similarity":
                assert abs(o["scale"][i] - c_ls) <= tol * max(1.0, c_ls), (P, i, o["scale"][i], c_ls)
                t = A.mean(0) - c_ls * R @ B.mean(0)
                assert np.abs(t - o["t"][i]).max() <= 1e-10 / max(o["kappa"][i], 1e-3)


def test_oracle_special_samples():
    x, entries = trajectory_case(40, n=8)
    o = oracle_trajectory(x, entries, "similarity")
    i = SPECIAL["exact"]
    assert abs(o["theta"][i] - np.pi / 2) <= 1e-15 and abs(o["scale"][i] - 2.0) <= 1e-14
    assert np.abs(o["t"][i] - [-30.0, 20.0]).max() <= 1e-12 and o["sse_traj"][i] <= 1e-22
    none = oracle_trajectory(x, entries, "none")
    assert none["sse_traj"][SPECIAL["truth"]] == 0.0 and none["sse_heading"][SPECIAL["truth"]] == 0.0
    assert none["sse_landmark"][SPECIAL["truth"]] == 0.0
    refl = oracle_trajectory(x, entries, "rigid", reflect=True)
    assert refl["reflected"][SPECIAL["mirrored"]] and refl["sse_traj"][SPECIAL["mirrored"]] <= 1e-22
    assert refl["sse_heading"][SPECIAL["mirrored"]] <= 1e-12
    assert not refl["reflected"][0] and not refl["reflected"][SPECIAL["truth"]]
    off = oracle_trajectory(x, entries, "rigid")
    assert off["sse_traj"][SPECIAL["mirrored"]] > 1.0 and not off["reflected"].any()
    # headings lie on both sides of the seam
    th = x[:, 2::3]
    assert th.max() > 3.0 and th.min() < -3.0


def test_oracle_equals_the_reference_outputs():
    """tests/golden/trajectory_error.npz: the reference's own kabsch_umeyama.  Its R is the oracle's R(theta); its scale is
    sum |a'|^2 / g and its t follows from that scale; its RMSE is reproduced by applying the oracle's rotation with them."""
    fx = np.load(os.path.join(GOLDEN, "trajectory_error.npz"))
    assert [str(s) for s in fx["names"]] == ["two", "three", "forty", "far", "nearly_pi"]
    for name in (str(s) for s in fx["names"]):
        A, B = fx["A_" + name], fx["B_" + name]
        assert B.dtype == np.float32 and A.dtype == np.float64
        P = len(A)
        cols = 2 * np.arange(P)
        entries = nh.pack_traj_entries(cols, cols + 1, np.full(P, -1), A)
        o = oracle_trajectory(B.reshape(1, -1), entries, "similarity")
        cs, sn = math.cos(o["theta"][0]), math.sin(o["theta"][0])
        R = np.array([[cs, -sn], [sn, cs]])
        assert np.abs(R - fx["R_" + name]).max() <= 1e-13, name
        c_ref = o["saa"][0] / o["g"][0]
        assert abs(c_ref - float(fx["c_" + name])) <= 1e-12 * c_ref, name
        B64 = B.astype(np.float64)
        t = A.mean(0) - c_ref * R @ B64.mean(0)
        assert np.abs(t - fx["t_" + name]).max() <= 1e-10, name
        rmse = np.sqrt(np.mean(np.sum((A - (c_ref * B64 @ R.T + t)) ** 2, axis=1)))
        assert abs(rmse - float(fx["rmse_" + name])) <= 1e-10 + 1e-12 * rmse, name
    assert abs(abs(math.atan2(fx["R_nearly_pi"][1, 0], fx["R_nearly_pi"][0, 0])) - np.pi) < 0.01
    assert np.abs(fx["A_far"]).min() > 50 and float(fx["rmse_far"]) < 0.05


def ill_conditioned_cases():
    """[(name, x [1, cols], entries)]: a near-collinear trajectory at 100 m (the second singular value of the SVD route is
    almost 0: the closed form does not care), and a mirrored loop graded with reflect off (dot and cross cancel:
    kappa = g / (|a'| |b'|) is a few per cent, the rotation is sensitive)."""
    rng = np.random.RandomState(5)
    P = 24
    s = np.linspace(-40.0, 40.0, P)
    a = np.stack([100.0 + s, 100.0 + 0.5 * s + 1e-4 * rng.standard_normal(P)], axis=1)
    b = a + 0.01 * rng.standard_normal((P, 2))
    ath = np.full(P, math.atan2(0.5, 1.0))
    cols = 3 * np.arange(P)
    x1 = np.zeros((1, 3 * P), dtype=np.float32)
    x1[0, 0::3], x1[0, 1::3], x1[0, 2::3] = b[:, 0], b[:, 1], ath + 0.01 * rng.standard_normal(P)
    e1 = nh.pack_traj_entries(cols, cols + 1, cols + 2, a, ath)
    ang = np.linspace(0.0, 2.0 * np.pi, P, endpoint=False)
    a2 = np.stack([100.0 + 30.0 * np.cos(ang), 100.0 + 29.0 * np.sin(ang)], axis=1)
    b2 = np.stack([a2[:, 0], 200.0 - a2[:, 1]], axis=1) + 0.01 * rng.standard_normal((P, 2))
    x2 = np.zeros((1, 3 * P), dtype=np.float32)
    x2[0, 0::3], x2[0, 1::3], x2[0, 2::3] = b2[:, 0], b2[:, 1], wrap_pi(-ang)
    e2 = nh.pack_traj_entries(cols, cols + 1, cols + 2, a2, wrap_pi(ang))
    return [("collinear", x1, e1), ("mirrored_loop", x2, e2)]


def test_oracle_equals_mpmath_on_ill_conditioned_cases():
    for name, x, entries in ill_conditioned_cases():
        for mode in ("rigid", "similarity"):
            o = oracle_trajectory(x, entries, mode)
            theta, c, t, ate, hrms, _, kappa = mp_trajectory(x[0], entries, mode)
            b = bounds(o, entries)
            print(name, mode, "kappa", kappa, "theta", o["theta"][0], theta, "ate", ate)
            assert abs(o["kappa"][0] - kappa) <= 1e-12
            assert abs(wrap_pi(o["theta"][0] - theta)) <= b["theta"][0]
            assert abs(o["scale"][0] - c) <= b["scale"][0]
            assert max(abs(o["t"][0][0] - t[0]), abs(o["t"][0][1] - t[1])) <= b["t"][0]
            got = math.sqrt(o["sse_traj"][0] / entries.size)
            assert abs(got - ate) <= b["resid"][0] + b["rel"] * ate
            assert abs(math.sqrt(o["sse_heading"][0] / entries.size) - hrms) <= b["heading"][0] + b["rel"] * hrms
        if name == "mirrored_loop":
            assert kappa < 0.1
        else:
            assert kappa > 0.99


# ---- kabsch_umeyama ---------------------------------------------------------------------------------------------------------------
def test_kabsch_umeyama_equals_the_reference_outputs():
    fx = np.load(os.path.join(GOLDEN, "trajectory_error.npz"))
    for name in (str(s) for s in fx["names"]):
        A, B = fx["A_" + name], fx["B_" + name].astype(np.float64)
        R, c, t = FN.kabsch_umeyama(A, B)
        assert np.abs(R - fx["R_" + name]).max() <= 1e-13 and abs(c - float(fx["c_" + name])) <= 1e-12 * c, name
        assert np.abs(t - fx["t_" + name]).max() <= 1e-10, name
        rmse = np.sqrt(np.mean(np.sum((A - (c * B @ R.T + t)) ** 2, axis=1)))
        assert abs(rmse - float(fx["rmse_" + name])) <= 1e-10 + 1e-12 * rmse, name


def test_kabsch_umeyama_recovers_an_exact_similarity_and_the_two_scale_rules_then_agree():
    rng = np.random.RandomState(1)
    for m in (2, 3):
        B = rng.standard_normal((9, m)) * 4.0
        Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
        if np.linalg.det(Q) < 0:
            Q[:, -1] = -Q[:, -1]
        c0, t0 = 1.75, rng.standard_normal(m) * 10.0
        A = c0 * B @ Q.T + t0
        R, c, t = FN.kabsch_umeyama(A, B)
        assert np.abs(R - Q).max() <= 1e-13 and abs(c - c0) <= 1e-13 and np.abs(t - t0).max() <= 1e-12
        da, db = A - A.mean(0), B - B.mean(0)
        g = np.sum(da * (db @ R.T))
        assert abs(np.sum(da * da) / g - g / np.sum(db * db)) <= 1e-13          # reference rule == least squares
    # with noise the reference's rule is the larger one
    A = A + 0.3 * rng.standard_normal(A.shape)
    R, c, _ = FN.kabsch_umeyama(A, B)
    da, db = A - A.mean(0), B - B.mean(0)
    assert c > np.sum(da * (db @ R.T)) / np.sum(db * db)
    with pytest.raises(ValueError, match="shape"):
        FN.kabsch_umeyama(np.zeros((3, 2)), np.zeros((4, 2)))


def test_kabsch_umeyama_on_a_mirrored_set():
    B = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 1.0], [1.0, 3.0]])            # not collinear
    A = B * np.array([1.0, -1.0]) + np.array([2.0, 5.0])
    R, c, t = FN.kabsch_umeyama(A, B)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14                                 # proper: the mirror is not undone
    assert np.sqrt(np.mean(np.sum((A - (c * B @ R.T + t)) ** 2, axis=1))) > 0.5
    R, c, t = FN.kabsch_umeyama(A, B, reflect=True)
    assert abs(np.linalg.det(R) + 1.0) <= 1e-14 and abs(c - 1.0) <= 1e-14
    assert np.abs(A - (c * B @ R.T + t)).max() <= 1e-13
    # the oracle on the same set: reflect off equals the proper SVD fit, on takes the mirror
    entries = nh.pack_traj_entries([0, 2, 4, 6], [1, 3, 5, 7], [-1] * 4, A)
    x = B.reshape(1, -1).astype(np.float32)
    off, on = oracle_trajectory(x, entries, "rigid"), oracle_trajectory(x, entries, "rigid", reflect=True)
    Rp, _, _ = FN.kabsch_umeyama(A, B)
    assert abs(math.cos(off["theta"][0]) - Rp[0, 0]) <= 1e-14 and abs(math.sin(off["theta"][0]) - Rp[1, 0]) <= 1e-14
    assert on["reflected"][0] and on["sse_traj"][0] <= 1e-25 and not off["reflected"][0]


# ---- the host summary ---------------------------------------------------------------------------------------------------------------
def test_trajectory_error_summary():
    ate = np.array([0.5, 0.1, 3.0, np.nan, 0.2])
    s = ST.trajectory_error_summary(ate, quantiles=(0.0, 0.5, 1.0), threshold=0.3)
    assert s["n"] == 5 and s["n_nan"] == 1 and s["best"] == (1, 0.1) and s["ess"] == 4.0
    assert abs(s["mean"] - 0.95) <= 1e-15 and s["below"] == 0.5
    assert s["quantiles"] == {0.0: 0.1, 0.5: 0.35, 1.0: 3.0}
    w = np.array([1.0, 0.0, 1.0, 5.0, 2.0])
    s = ST.trajectory_error_summary(ate, w, quantiles=(0.5,), threshold=1.0)
    assert s["best"] == (4, 0.2) and abs(s["mean"] - (0.5 + 3.0 + 0.4) / 4.0) <= 1e-15 and s["below"] == 0.75
    assert abs(s["ess"] - 16.0 / 6.0) <= 1e-15 and s["quantiles"] == {0.5: 0.2}
    assert ST.trajectory_error_summary(ate)["below"] is None
    assert ST.trajectory_error_summary(np.array([np.nan]))["ess"] == 0.0
    for bad in (dict(weights=np.ones(4)), dict(weights=-np.ones(5)), dict(weights=np.zeros(5)), dict(quantiles=(1.5,))):
        with pytest.raises(ValueError):
            ST.trajectory_error_summary(ate, **bad)
    with pytest.raises(ValueError, match="no samples"):
        ST.trajectory_error_summary(np.zeros(0))
    assert np.array_equal(ST.weighted_quantiles([3.0, 1.0, 2.0], [0.5]), [2.0])
    assert np.array_equal(ST.weighted_quantiles([3.0, 1.0, 2.0], [0.0, 0.5, 1.0], [1.0, 1.0, 6.0]), [1.0, 2.0, 3.0])


# ---- the surface --------------------------------------------------------------------------------------------------------------------
NEW = ("nfisam_sample_trajectory_error", "nfisam_sample_trajectory_rpe", "nfisam_sample_trajectory_scratch_count")


def test_library_exports_the_new_entries_and_the_abi_version_stays():
    nh.build()
    lib = nh.lib()
    for name in NEW:
        assert name in nh.EXPORTS and hasattr(lib, name), name
    assert lib.nfisam_abi_version() == 1600
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    for name in NEW:
        assert name + "(" in hdr
    assert "Functions.py:53-71" in hdr and "plaza_traj_performance_plot.py:112-114,196-198,282-293" in hdr
    assert "sample_trajectory.hip" in open(os.path.join(ROOT, "nf-isam_amd", "csrc", "sample_common.h")).read()
    assert "sample_trajectory" in open(os.path.join(ROOT, "nf-isam_amd", "csrc", "Makefile")).read()
    assert lib.nfisam_sample_trajectory_scratch_count(130, 5) == 3 * 6 and lib.nfisam_sample_trajectory_scratch_count(0, 5) == 0
    for f in (nh.pack_traj_entries, nh.check_traj_entries, nh.pack_traj_pairs, nh.check_traj_pairs, nh.sample_trajectory_error,
              nh.sample_trajectory_error_t, nh.sample_trajectory_rpe, nh.sample_trajectory_rpe_t, ST.trajectory_error,
              ST.trajectory_error_t, ST.relative_pose_error, ST.trajectory_error_summary, FN.kabsch_umeyama):
        assert callable(f)
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_trajectory_error is NFiSAM.posterior_trajectory_error


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfisam_hip.h"\nint main(void) { '
                   'printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(nfisam_traj_entry), offsetof(nfisam_traj_entry, flags), '
                   'offsetof(nfisam_traj_entry, ax), offsetof(nfisam_traj_entry, ath), sizeof(nfisam_traj_pair), '
                   'offsetof(nfisam_traj_pair, slot), NFISAM_TRAJ_ALIGNED, NFISAM_TRAJ_LANDMARK, NFISAM_TRAJ_ALIGN_NONE, '
                   'NFISAM_TRAJ_ALIGN_RIGID, NFISAM_TRAJ_ALIGN_SIMILARITY, NFISAM_TRAJ_OUT_ROWS); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [40, 12, 16, 32, 16, 8, 1, 2, 0, 1, 2, 8]
    assert sizes[:4] == [C.sizeof(nh.TrajEntry), nh.TrajEntry.flags.offset, nh.TrajEntry.ax.offset, nh.TrajEntry.ath.offset]
    assert [nh.TRAJ_ENTRY_DTYPE.fields[k][1] for k in ("col_x", "col_y", "col_th", "flags", "ax", "ay", "ath")] == [0, 4, 8, 12, 16, 24, 32]
    assert [nh.TRAJ_PAIR_DTYPE.fields[k][1] for k in ("i", "j", "slot", "reserved")] == [0, 4, 8, 12]
    assert (nh.TRAJ_ALIGNED, nh.TRAJ_LANDMARK, nh.TRAJ_OUT_ROWS) == (1, 2, 8)
    assert nh.TRAJ_MODES == {"none": 0, "rigid": 1, "similarity": 2}


def _entries3():
    return nh.pack_traj_entries([0, 3, 6], [1, 4, 7], [2, 5, -1], np.arange(6.0).reshape(3, 2), [0.1, 0.2, 0.0],
                                landmark=[False, False, True])


def test_host_side_refusals_of_the_c_entries():
    """Both entries refuse bad arguments on the host, before they touch the device (the pointers below are never
    dereferenced: they are not device memory)."""
    nh.build()
    lib = nh.lib()
    fake = C.c_void_p(4096)
    good = _entries3()

    def error(Xt=fake, rows=8, n=5, ent=good, ent_dev=fake, P=3, mode=1, out=fake, iout=fake, sums=fake, scratch=fake):
        return lib.nfisam_sample_trajectory_error(Xt, rows, n, None if ent is None else ent.ctypes.data_as(C.c_void_p), ent_dev, P,
                                                  mode, 0, None, out, iout, sums, scratch, None)
    for kw in (dict(Xt=None), dict(ent=None), dict(ent_dev=None), dict(out=None), dict(iout=None), dict(sums=None),
               dict(scratch=None), dict(n=0), dict(n=-2), dict(P=0), dict(P=-1), dict(rows=0), dict(mode=3), dict(mode=-1),
               dict(rows=7)):
        assert error(**kw) == nh.ERR_ARG, kw
    for field, value in (("col_x", -1), ("col_x", 8), ("col_y", 8), ("col_th", -2), ("col_th", 8), ("flags", 4), ("ax", np.nan),
                         ("ay", np.inf), ("ath", np.nan)):
        bad = good.copy()
        bad[field][0] = value
        assert error(ent=bad) == nh.ERR_ARG, (field, value)
    none_aligned = good.copy()
    none_aligned["flags"] &= ~1
    assert error(ent=none_aligned, mode=1) == nh.ERR_ARG and error(ent=none_aligned, mode=2) == nh.ERR_ARG

    pairs = nh.pack_traj_pairs([0, 1], [1])

    def rpe(Xt=fake, rows=8, n=5, ent=good, ent_dev=fake, P=3, pr=pairs, pr_dev=fake, npairs=1, slots=1, out=fake):
        return lib.nfisam_sample_trajectory_rpe(Xt, rows, n, None if ent is None else ent.ctypes.data_as(C.c_void_p), ent_dev, P,
                                                None if pr is None else pr.ctypes.data_as(C.c_void_p), pr_dev, npairs, slots, out,
                                                None)
    for kw in (dict(Xt=None), dict(ent=None), dict(ent_dev=None), dict(pr=None), dict(pr_dev=None), dict(out=None), dict(n=0),
               dict(P=0), dict(rows=0), dict(npairs=0), dict(slots=0), dict(slots=65536), dict(rows=5)):
        assert rpe(**kw) == nh.ERR_ARG, kw
    for field, value in (("i", -1), ("i", 3), ("j", 3), ("j", 2), ("slot", 1), ("slot", -1)):      # entry 2 has no heading
        bad = pairs.copy()
        bad[field][0] = value
        assert rpe(pr=bad) == nh.ERR_ARG, (field, value)


def test_tables_pack_and_their_checks_refuse():
    t = _entries3()
    assert list(t["flags"]) == [1, 1, 2] and list(t["col_th"]) == [2, 5, -1] and list(t["ax"]) == [0.0, 2.0, 4.0]
    assert list(t["ath"]) == [0.1, 0.2, 0.0]
    assert nh.check_traj_entries(t, 8) == 1 and nh.check_traj_entries(t, 8, "none") == 0 and nh.check_traj_entries(t, 8, "similarity") == 2
    t2 = nh.pack_traj_entries([0], [1], [-1], [[1.0, 2.0]], aligned=[False], landmark=[False])
    assert int(t2["flags"][0]) == 0
    nh.check_traj_entries(t2, 2, "none")
    with pytest.raises(ValueError, match="aligned entry"):
        nh.check_traj_entries(t2, 2, "rigid")
    with pytest.raises(ValueError, match="align is one of"):
        nh.check_traj_entries(t, 8, "affine")
    with pytest.raises(ValueError, match="TRAJ_ENTRY_DTYPE"):
        nh.check_traj_entries(np.zeros(3), 8)
    with pytest.raises(ValueError, match="P >= 1"):
        nh.check_traj_entries(t[:0], 8)
    with pytest.raises(ValueError, match="out of range"):
        nh.check_traj_entries(t, 7)
    for field, value, match in (("col_x", -1, "out of range"), ("col_th", -2, "out of range"), ("col_th", 9, "out of range"),
                                ("flags", 4, "unknown flag"), ("ax", np.nan, "finite"), ("ath", np.inf, "finite")):
        bad = t.copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match=match):
            nh.check_traj_entries(bad, 8)
    with pytest.raises(ValueError, match="one row triple"):
        nh.pack_traj_entries([0, 1], [1], [-1, -1], np.zeros((2, 2)))
    p = nh.pack_traj_pairs([4, 7, 9, 11], [1, 3])
    assert [tuple(r) for r in p] == [(4, 7, 0, 0), (7, 9, 0, 0), (9, 11, 0, 0), (4, 11, 1, 0)]
    for strides in ([0], [4], [-1]):
        with pytest.raises(ValueError, match="stride"):
            nh.pack_traj_pairs([4, 7, 9, 11], strides)
    with pytest.raises(ValueError, match="no stride"):
        nh.pack_traj_pairs([4, 7], [])
    ok = nh.pack_traj_pairs([0, 1], [1])
    assert nh.check_traj_pairs(ok, t) == 1 and nh.check_traj_pairs(ok, t, 3) == 3
    for field, value, match in (("i", 3, "outside the 3 entries"), ("j", -1, "outside"), ("j", 2, "no heading"), ("slot", 2, "slot")):
        bad = ok.copy()
        bad[field][0] = value
        with pytest.raises(ValueError, match=match):
            nh.check_traj_pairs(bad, t, 2)
    with pytest.raises(ValueError, match="TRAJ_PAIR_DTYPE"):
        nh.check_traj_pairs(np.zeros(2), t)
    with pytest.raises(ValueError, match="at least one pair"):
        nh.check_traj_pairs(ok[:0], t)
    with pytest.raises(ValueError, match="slots"):
        nh.check_traj_pairs(ok, t, 65536)
    for strides, match in (([1, 1], "distinct"), ([], "non-empty"), ([1.5], "distinct integers"), ("a", "integers"), ([3], r"\[1, 3\)")):
        with pytest.raises(ValueError, match=match):
            ST.check_strides(strides, 3)
    assert ST.check_strides([1, 2], 3) == (1, 2)


class Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


def test_cpu_tensors_and_bad_arguments_are_refused_before_any_launch(monkeypatch):
    refuse = Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    t = _entries3()
    pairs = nh.pack_traj_pairs([0, 1], [1])
    X = torch.zeros(5, 8)
    for call in (lambda: nh.sample_trajectory_error(X, t), lambda: nh.sample_trajectory_error(X.numpy(), t, device="cpu"),
                 lambda: nh.sample_trajectory_error_t(X.t().contiguous(), t), lambda: nh.sample_trajectory_rpe(X, t, pairs),
                 lambda: nh.sample_trajectory_rpe_t(X.t().contiguous(), t, pairs),
                 lambda: ST.trajectory_error(X, np.zeros((2, 2)), np.zeros(2)),
                 lambda: ST.relative_pose_error(X, np.zeros((2, 2)), np.zeros(2))):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()
    x = X.numpy()
    with pytest.raises(ValueError, match="out of range"):
        nh.sample_trajectory_error(x[:, :7], t, device="cuda")
    with pytest.raises(ValueError, match="no points"):
        nh.sample_trajectory_error(x[:0], t, device="cuda")
    with pytest.raises(ValueError, match="align is one of"):
        nh.sample_trajectory_error(x, t, align="affine", device="cuda")
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        nh.sample_trajectory_error(np.zeros(5, dtype=np.float32), t, device="cuda")
    for w, match in ((np.ones(4), r"\[n\]"), (-np.ones(5), "non-negative"), (np.zeros(5), "all zero"),
                     (np.array([1, np.nan, 1, 1, 1.0]), "finite")):
        with pytest.raises(ValueError, match=match):
            nh.sample_trajectory_error(x, t, weights=w, device="cuda")
    bad = pairs.copy()
    bad["j"][0] = 2
    with pytest.raises(ValueError, match="no heading"):
        nh.sample_trajectory_rpe(x, t, bad, device="cuda")
    with pytest.raises(ValueError, match="no points"):
        nh.sample_trajectory_rpe(x[:0], t, pairs, device="cuda")
    with pytest.raises(ValueError, match="truth_xy"):
        ST.trajectory_error(x, np.zeros((0, 2)), device="cuda")
    with pytest.raises(ValueError, match="truth_th"):
        ST.trajectory_error(x, np.zeros((2, 2)), np.zeros(3), device="cuda")
    with pytest.raises(ValueError, match="pose_cols"):
        ST.trajectory_error(x, np.zeros((2, 2)), np.zeros(2), pose_cols=[[0, 1]], device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        ST.trajectory_error(x, np.zeros((3, 2)), np.zeros(3), device="cuda")                  # 9 columns needed, 8 there
    with pytest.raises(ValueError, match="landmark_xy"):
        ST.trajectory_error(x, np.zeros((2, 2)), np.zeros(2), landmark_cols=[[6, 7]], device="cuda")
    with pytest.raises(ValueError, match="columns"):
        ST.trajectory_error(np.zeros(5), np.zeros((2, 2)), device="cuda")
    with pytest.raises(ValueError, match="stride"):
        ST.relative_pose_error(x, np.zeros((2, 2)), np.zeros(2), strides=[2], device="cuda")
    with pytest.raises(ValueError, match="headings"):
        ST.relative_pose_error(x, np.zeros((2, 2)), None, device="cuda")
    entries, P = ST.trajectory_entries(8, np.zeros((2, 2)), np.zeros(2), landmark_xy=[[1.0, 2.0]])
    assert P == 2 and list(entries["col_x"]) == [0, 3, 6] and list(entries["col_th"]) == [2, 5, -1] and list(entries["flags"]) == [1, 1, 2]
    assert refuse.calls == 0


# ---- the solver -------------------------------------------------------------------------------------------------------------------
def test_posterior_trajectory_error_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    nh.build()
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().posterior_trajectory_error({})
    X0, X1, L1 = SE2Variable("X0"), SE2Variable("X1"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    for v in (X0, X1, L1):
        s.add_node(v)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X1, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    refuse = Refuse()
    for name in ("sample_trajectory_error", "sample_trajectory_error_t", "sample_trajectory_rpe", "sample_trajectory_rpe_t",
                 "sample_moments", "sample_moments_t", "posterior_walk_raw", "upload", "posterior_log_density",
                 "posterior_log_density_t", "factor_graph_log_density", "factor_graph_log_density_t"):
        monkeypatch.setattr(nh, name, refuse)
    own = {X0: np.zeros((7, 3)), X1: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    truth = {X0: np.zeros(3), X1: np.ones(3), L1: np.ones(2)}
    X9 = SE2Variable("X9")
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):      # a draw needs a trained tree
        s.posterior_trajectory_error(truth)
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):
        s.posterior_trajectory_error(truth, own, weights="importance")
    with pytest.raises(ValueError, match="truth holds none of the poses"):
        s.posterior_trajectory_error({L1: np.ones(2)}, own)
    with pytest.raises(ValueError, match="truth holds none of the poses"):
        s.posterior_trajectory_error({X9: np.ones(3)}, own, poses=[X0, X1])
    with pytest.raises(ValueError, match="truth lacks variable X1"):
        s.posterior_trajectory_error({X0: np.zeros(3)}, own, poses=[X0, X1])
    with pytest.raises(ValueError, match="X9 is not in the elimination ordering"):
        s.posterior_trajectory_error({**truth, X9: np.zeros(3)}, own, poses=[X0, X9])
    with pytest.raises(ValueError, match=r"truth of X1 must be \[3\]"):
        s.posterior_trajectory_error({**truth, X1: np.zeros(2)}, own, poses=[X0, X1])
    for strides in ([2], [1, 5], [0]):
        with pytest.raises(ValueError, match="stride"):
            s.posterior_trajectory_error(truth, own, strides=strides)
    with pytest.raises(ValueError, match="align is one of"):
        s.posterior_trajectory_error(truth, own, align="affine")
    with pytest.raises(ValueError, match="'importance'"):
        s.posterior_trajectory_error(truth, own, weights="uniform")
    for w, match in ((np.ones(6), r"\[n\] = \[7\]"), (-np.ones(7), "non-negative"), (np.zeros(7), "all zero")):
        with pytest.raises(ValueError, match=match):
            s.posterior_trajectory_error(truth, own, weights=w)
    with pytest.raises(ValueError, match="probabilities"):
        s.posterior_trajectory_error(truth, own, quantiles=[1.5])
    with pytest.raises(ValueError, match="threshold"):
        s.posterior_trajectory_error(truth, own, threshold=0.0)
    with pytest.raises(ValueError, match="listed twice"):
        s.posterior_trajectory_error(truth, own, poses=[X0, X0], strides=())
    with pytest.raises(ValueError, match="heading on every pose"):
        s.posterior_trajectory_error(truth, own, poses=[X0, L1], landmarks=[])
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_trajectory_error(truth, {X0: own[X0], X1: own[X1]})
    with pytest.raises(ValueError, match="no points"):
        s.posterior_trajectory_error(truth, {v: a[:0] for v, a in own.items()})
    assert refuse.calls == 0
