"""Forward error of the density direction, element by element, in float64 -- the grader of tests/test_density_forward_gpu.py and
its own tests on the CPU.  Conventions, fixture, trees and the bound are those of tests/test_sampler_backward_cpu.py.

The density direction (nfisam_nsf_forward, nfisam_nsf_posterior_log_density) takes exact float32 points x and returns
z = flow(x), the log-det and a log-density.  The reference is `forward64` (per dim: fwd, lad summed over layers, d lad_i / d x_i
with the conditioning held fixed); slope_i = exp(lad_i):

    r_z[p, i] = |z - fwd64| / (2^-24 L s_z),    s_z  = (B + |fwd64|) + slope_i (B + |x_i|)
    r_ld[p]   = |ld - sum_i lad64| / (2^-24 L s_ld),   s_ld = sum_i (1 + |d lad_i / d x_i| (B + |x_i|))
    r_lp[p]   = |lp - lp64| / (2^-24 L (s_ld + sum_i (|fwd64_i| s_z,i + fwd64_i^2 / 2 + 0.92)))

`s_z` is what half an ulp of the quantities of size <= B + |.| on either side of the spline moves z by, `s_ld` the same for the
log-det (a sum of D terms of size ~1, each moved by its own x_i), and the prior -z^2 / 2 - 0.92 moves by |z| dz plus its own
rounding.  The forward spline and its derivative are continuous across knots, so either bin will do; tails are the identity.

A clique's term of the tree density: the row [obs | sep | frontal] is normalised in float64 as `backward_ratio` does
(wrap(x - mean) / std on angle columns), extra = (|x_raw| + |mean| + pi circular) / std joins (B + |x_i|): the rounding of the
normalisation; t64 = sum over the frontal dims of (lad64 - fwd64^2 / 2 - 1/2 log 2 pi - log std) -- a sum of the frontal dims'
own terms, NOT lp(D) - lp(Ds), which cancels; its scale is the r_lp scale over the frontal dims plus sum |log std|; r_lat is
r_z on the `latent` output; log_q is graded against sum_c t64 with the cliques' scales added.

The bound is not fixed here: every case also runs a float32 replay through the same grader -- `CO.forward(dtype=float32)` for
the flow, `O.layer_theta` / `O.rqs` in torch float32 with `O.normalize_samples`, summed per frontal column in float32, for a
clique's term.  Its largest ratio is R32;
    condition on the inputs   R32 <= 64
    bound on a kernel         max r <= 8 max(R32, 4) over EVERY element -- no quantile, no mask
(the factor 8: see tests/test_sampler_backward_cpu.py).  A NaN input that comes back NaN has ratio 0 (its bits are compared
apart), its row's log-density must be NaN; any other non-finite value has ratio inf.

Cases.  Forward: every un-normalised entry of INVERSE_CASES (the given columns are simply the leading ones: 14 distinct flows,
D = 1 .. 20, K = 2 .. 16, H = 4, 8, 16, L = 1 .. 3, model_D = 9 > D = 6), and d20h16 truncated to D = 2 (two waves: the sum still
commutes), 3 (the first sum whose order matters), 8 (eight waves) and 9 (wave 0 takes dims 0 and 8).  x = 1.6 randn, n = 130, with
planted rows: +-B and both float32 neighbours of each, +-7.5, 0, -4.9999 (once counted from the first column, once from the
last), NaN in the last column only (nothing conditions on it), one row with every column in a tail (its log-det is exactly 0),
and in dim 0 the float32 values at and 1, 2 ulps around every interior width knot of the first layer.  Tree density: the six
WALK_TREES at `walk_reference(name)["S"]` (tail and box-edge draws included), rows with every angle column shifted by +-2 pi and
rows with one frontal and one separator column 6.5 std from its mean (beyond B; angle columns have std <= 0.4, so that stays
0.5 away from the seam mean +- pi, where a point lands on either side legitimately).

Measured on the float32 replays (`test_*_meets_the_condition` print every case's; the MI355X's figures are in
profiles/density_forward_error.json): forward R32 of r_z 1.8 .. 6.1, of r_ld 1.0 .. 24.6 (largest at D = 1, then D = 2: few terms
in s_ld), of r_lp 0.6 .. 2.4; a clique's term 0.4 .. 3.3, its latent 1.1 .. 3.7, log_q 0.3 .. 0.8.  The torch replay of the
tree terms depends on the host's float32 vector code: another host read 0.4 .. 4.7 on the terms.

The CPU tests below grade the grader: mutations of the float32 replay's output that a wrong kernel would produce must each
exceed the bound.  One cannot be told apart everywhere and is asserted only where it can: the neighbouring bin's
rational-quadratic (the point's own left knots, every other quantity of the bin to the right) moves z by nothing when the point
sits ON the knot or within 2 ulps to its right (t ~ 0), there only the log-det shows it (the derivative of the wrong bin's left
end), and a point 1 or 2 ulps to the LEFT of the knot is in the bin before it, whose neighbour is far off in z as well."""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import nsf_torch as O
from test_sampler_backward_cpu import (B, EPS32, INVERSE_CASES, N, R32_MAX, SPECIALS, WALK_TREES, _shape, bound, fixture, forward64,
                                       truncated, walk_reference, walk_tree)

HALF_LOG_2PI = 0.9189385332046727


def _wrap(t):
    return (t + np.pi) % (2 * np.pi) - np.pi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ratio(err, scale):
    r = err / scale
    return np.where(np.isfinite(r), r, np.inf)


# ------------------------------------------------------------------ forward: cases -------
FCase = namedtuple("FCase", "name blob model_D D K H L seed")


def forward_cases():
    out, seen = [], set()
    for c in INVERSE_CASES:
        if c.norm or (c.blob, c.D) in seen:
            continue
        seen.add((c.blob, c.D))
        out.append(FCase("%s-D%d" % (c.blob, c.D), c.blob, c.model_D, c.D, c.K, c.H, c.L, 3000 + len(out)))
    mD, K, H, L = _shape("d20h16")
    for D in (2, 3, 8, 9):
        out.append(FCase("d20h16-D%d" % D, "d20h16", mD, D, K, H, L, 3100 + D))
    return out


FORWARD_CASES = forward_cases()
FORWARD_IDS = [c.name for c in FORWARD_CASES]
assert len(FORWARD_CASES) == 18


def fcase(name):
    return FORWARD_CASES[FORWARD_IDS.index(name)]


def case_blob(c):
    return truncated(fixture()["blob_" + c.blob], c.model_D, c.D, c.K, c.H, c.L)


def width_knots(init_param, K):
    """Interior knots of the width spline of a shared theta, in float64."""
    th = torch.as_tensor(np.asarray(init_param), dtype=torch.float64)
    cw, _ = O._knots(th[:K], K, B, O.MIN_W)
    return cw.numpy()[1:-1]


def around(y):
    """The float32 values at and 1, 2 ulps around y."""
    v = np.float32(y)
    lo1, hi1 = np.nextafter(v, np.float32(-9)), np.nextafter(v, np.float32(9))
    return [np.nextafter(lo1, np.float32(-9)), lo1, v, hi1, np.nextafter(hi1, np.float32(9))]


@functools.lru_cache(maxsize=None)
def forward_inputs(name):
    """-> (x [N, D] float32, knot_rows: the rows whose dim 0 sits within 2 ulps of an interior width knot of layer 0, all_tail: the
    row whose every column is in a tail)."""
    c = fcase(name)
    rng = np.random.RandomState(c.seed)
    x = (1.6 * rng.randn(N, c.D)).astype(np.float32)
    row = 0
    for rev in (False, True):
        for j, v in enumerate(SPECIALS):
            col = c.D - 1 if np.isnan(v) else (c.D - 1 - j % c.D if rev else j % c.D)
            x[row, col] = v
            row += 1
    all_tail = row
    x[row] = np.where(np.arange(c.D) % 2 == 0, 7.5, -6.25).astype(np.float32)
    row += 1
    first = row
    for y in width_knots(case_blob(c)[:3 * c.K - 1], c.K):
        for u in around(y):
            x[row, 0] = u
            row += 1
    assert row <= N
    x.setflags(write=False)
    return x, np.arange(first, row), all_tail


# ------------------------------------------------------------------ forward: the grader --
def forward_scales(x32, blob, K, H, L, extra=None, xn=None):
    """float64 reference and scales at the exact float32 rows x32 (or at the float64 rows xn normalised from them, with
    `extra` [n, D] joining B + |x|) -> dict of fwd, lad, s_z [n, D] and, per dim, the log-det and log-density scale terms."""
    x = np.asarray(x32, dtype=np.float64) if xn is None else xn
    nan = np.isnan(x)
    xe = np.where(nan, 2 * B, x)                          # a tail value: identity, log-det 0, conditions nothing here
    fwd, lad, dlad = forward64(xe, blob, K, H, L)
    mag = B + np.abs(xe) + (0.0 if extra is None else extra)
    s_z = (B + np.abs(fwd)) + np.exp(lad) * mag
    s_ld = 1.0 + np.abs(dlad) * mag
    s_pr = np.abs(fwd) * s_z + 0.5 * fwd * fwd + 0.92
    return dict(nan=nan, fwd=fwd, lad=lad, s_z=s_z, s_ld=s_ld, s_pr=s_pr, L=L)


def forward_ratio(ref, z=None, ld=None, lp=None):
    """-> (r_z [n, D], r_ld [n], r_lp [n]) (None for the outputs not given) against `forward_scales`' reference."""
    D, eps = ref["fwd"].shape[1], EPS32 * ref["L"]
    r_z = r_ld = r_lp = None
    if z is not None:
        z = np.asarray(z, dtype=np.float64)
        pair = ref["nan"] & np.isnan(z)
        r_z = _ratio(np.abs(np.where(pair, 2 * B, z) - ref["fwd"]), eps * ref["s_z"])
    if ld is not None:
        r_ld = _ratio(np.abs(np.asarray(ld, dtype=np.float64) - ref["lad"].sum(1)), eps * ref["s_ld"].sum(1))
    if lp is not None:
        lp = np.asarray(lp, dtype=np.float64)
        lp64 = ref["lad"].sum(1) - 0.5 * (ref["fwd"] ** 2).sum(1) - D * HALF_LOG_2PI
        pair = ref["nan"].any(1) & np.isnan(lp)            # a NaN column: the row's density is NaN
        r_lp = _ratio(np.abs(np.where(pair, lp64, lp) - lp64), eps * (ref["s_ld"].sum(1) + ref["s_pr"].sum(1)))
        r_lp = np.where(ref["nan"].any(1) & ~pair, np.inf, r_lp)
    return r_z, r_ld, r_lp


def logprob32(z, ld):
    """The kernel's own closing line in float32: the squares added in dim order."""
    z = np.asarray(z, dtype=np.float32)
    zz = np.zeros(z.shape[0], dtype=np.float32)
    for k in range(z.shape[1]):
        zz = zz + z[:, k] * z[:, k]
    return np.float32(-0.5) * zz - np.float32(0.5) * np.float32(z.shape[1]) * np.float32(2 * HALF_LOG_2PI) + np.asarray(ld, dtype=np.float32)


def oracle_forward(c, x, dtype=np.float32, blob=None):
    """The project's oracle on the case -> (z, ld, lp) float32."""
    z, ld = CO.forward(np.asarray(x), case_blob(c) if blob is None else blob, c.K, c.H, B, c.L, dtype=dtype)
    if dtype == np.float64:
        lp = ld - 0.5 * (z * z).sum(1) - c.D * HALF_LOG_2PI
        return z.astype(np.float32), ld.astype(np.float32), lp.astype(np.float32)
    return z, ld, logprob32(z, ld)


def exact_failures(x, z, ld, lp, L):
    """The tolerance-free properties of one forward call -> list of messages (empty: all hold)."""
    x, z = np.asarray(x, dtype=np.float32), np.asarray(z, dtype=np.float32)
    tail = ~(np.abs(x) <= np.float32(B))
    nanrow = np.isnan(x).any(1)
    bad = []
    if not np.array_equal(_bits(z)[tail], _bits(x)[tail]):
        bad.append("a tail / NaN column did not come through with its own bits")
    if not np.all(np.isfinite(z[~tail])):
        bad.append("non-finite z inside the box")
    if not np.all(np.isfinite(ld)):
        bad.append("non-finite log-det")
    if not np.all(np.isfinite(np.asarray(lp)[~nanrow])) or not np.all(np.isnan(np.asarray(lp)[nanrow])):
        bad.append("log-density not finite, or not NaN in a row with a NaN column")
    whole = tail.all(1)                                   # every column in a tail: the identity in every layer, each dim adds 0
    if not np.all(np.asarray(ld)[whole] == 0.0):
        bad.append("a row of tail columns has a log-det other than 0")
    return bad


PLACES = (slice(0, 1), slice(0, 64), slice(0, 65), slice(N - 1, N), slice(0, N))


@functools.lru_cache(maxsize=None)
def forward_reference(name):
    """Inputs, the float64 reference with its scales and the float32 oracle's outputs and ratios, once per case (shared: callers
    must not modify them)."""
    c = fcase(name)
    x, knot_rows, all_tail = forward_inputs(name)
    ref = forward_scales(x, case_blob(c), c.K, c.H, c.L)
    z, ld, lp = oracle_forward(c, x)
    r_z, r_ld, r_lp = forward_ratio(ref, z, ld, lp)
    return dict(x=x, knot_rows=knot_rows, all_tail=all_tail, ref=ref, z=z, ld=ld, lp=lp, R32_z=float(r_z.max()),
                R32_ld=float(r_ld.max()), R32_lp=float(r_lp.max()))


# ------------------------------------------------------------------ the tree density -----
ONE_WAVE_TREES = ["tree-l1h8", "tree-l2h8", "tree-l1h4"]
ONE_WAVE_COPIES = 2700
DENSITY_TILE, DENSITY_BLOCKS_4_WAVES = 64, 16384


def density_waves(n, n_cliques):
    """`unit_density`: `const int W = (blocks <= 16384) ? DENS_WAVES : 1;` with blocks = tiles of 64 points x cliques
    -> (waves per block, blocks)."""
    blocks = -(-n // DENSITY_TILE) * n_cliques
    return (4 if blocks <= DENSITY_BLOCKS_4_WAVES else 1), blocks


@functools.lru_cache(maxsize=None)
def tree_points(name):
    """X [n, total] float32: the walk's draws S, then 12 rows of S with every angle column (of any clique) + 2 pi, 12 with - 2 pi,
    then per clique one row with its first frontal and one with its first separator column 6.5 std from the mean (as that clique
    normalises the column; sign alternating)."""
    K, H, L, total, cliques = walk_tree(name)
    S = walk_reference(name)["S"]
    angle = np.zeros(total, dtype=bool)
    for q in cliques:
        Ds = len(q.obs) + len(q.sep)
        for k, col in enumerate(q.sep + q.front):
            angle[col] |= bool(q.circ[len(q.obs) + k])
    up, dn = S[:12].copy(), S[12:24].copy()
    up[:, angle] += np.float32(2 * np.pi)
    dn[:, angle] -= np.float32(2 * np.pi)
    far, r = S[24:24 + 2 * len(cliques)].copy(), 0
    for j, q in enumerate(cliques):
        Ds = len(q.obs) + len(q.sep)
        for k, col in ((Ds, q.front[0]),) + (((len(q.obs), q.sep[0]),) if q.sep else ()):
            far[r, col] = np.float32(q.mean[k]) + np.float32(6.5 if (j + r) % 2 else -6.5) * np.float32(q.std[k])
            r += 1
    X = np.concatenate([S, up, dn, far[:r]]).astype(np.float32)
    X.setflags(write=False)
    return X, angle


def clique_row(q, X, obs=None):
    n = X.shape[0]
    o = np.tile(q.obs, (n, 1)) if obs is None else obs
    return np.concatenate([o, X[:, q.sep], X[:, q.front]], 1).astype(np.float32)


def clique_scales(q, K, H, L, X):
    """One clique's float64 reference at the points X [n, total] float32 -> dict(t64 [n], scale [n], fwd [n, F], s_z [n, F])."""
    Ds, F = len(q.obs) + len(q.sep), len(q.front)
    D = Ds + F
    row = clique_row(q, X).astype(np.float64)
    mean, std, circ = q.mean[:D].astype(np.float64), q.std[:D].astype(np.float64), q.circ[:D].astype(bool)
    d = row - mean
    xn = np.where(circ, _wrap(d), d) / std
    extra = (np.abs(row) + np.abs(mean) + np.pi * circ) / std
    ref = forward_scales(None, truncated(q.blob, q.D_model, D, K, H, L), K, H, L, extra=extra, xn=xn)
    assert not ref["nan"].any()
    f = slice(Ds, D)
    fwd, logstd = ref["fwd"][:, f], np.log(std[f])
    t64 = (ref["lad"][:, f] - 0.5 * fwd * fwd - HALF_LOG_2PI - logstd).sum(1)
    scale = ref["s_ld"][:, f].sum(1) + ref["s_pr"][:, f].sum(1) + np.abs(logstd).sum()
    return dict(t64=t64, scale=scale, fwd=fwd, s_z=ref["s_z"][:, f], L=L)


def tree_ratio(refs, per, latent=None, log_q=None):
    """refs: `clique_scales` of every clique in table order; per [n_cliques, n], latent [>= sum F, n] (rows in walk order), log_q [n]
    -> ([largest r_per per clique], [largest r_lat per clique] or None, largest r of log_q or None)."""
    eps = EPS32 * refs[0]["L"]
    r_per = [float(_ratio(np.abs(np.asarray(p, dtype=np.float64) - r["t64"]), eps * r["scale"]).max()) for r, p in zip(refs, per)]
    r_lat = None
    if latent is not None:
        r_lat, zrow = [], 0
        for r in refs:
            F = r["fwd"].shape[1]
            r_lat.append(float(_ratio(np.abs(np.asarray(latent[zrow:zrow + F], dtype=np.float64).T - r["fwd"]), eps * r["s_z"]).max()))
            zrow += F
    r_q = None
    if log_q is not None:
        r_q = float(_ratio(np.abs(np.asarray(log_q, dtype=np.float64) - sum(r["t64"] for r in refs)),
                           eps * sum(r["scale"] for r in refs)).max())
    return r_per, r_lat, r_q


SUM_WAVES = 16


def sum_in_table_order(per):
    """`nsf_density_sum_kernel` in float32: the cliques are cut into SUM_WAVES contiguous runs of ceil(n_cliques / SUM_WAVES), each
    run is added in order starting from 0.0f, then the runs' sums are added in run order."""
    per = np.asarray(per, dtype=np.float32)
    nc, n = per.shape
    run = -(-nc // SUM_WAVES)
    total = None
    for w in range(SUM_WAVES):
        s = np.zeros(n, dtype=np.float32)
        for c in range(w * run, min((w + 1) * run, nc)):
            s = s + per[c]
        total = s if total is None else total + s
    return total


def replay_clique32(q, K, H, L, X, mut=None):
    """The float32 replay of one clique's term (torch float32, `O.normalize_samples`) -> (per [n], latent [n, F]) or, with `mut`,
    what a kernel with that defect would return."""
    Ds, F = len(q.obs) + len(q.sep), len(q.front)
    D = Ds + F
    obs = X[:, :len(q.obs)] if mut == "obs-from-point" else None
    row = clique_row(q, X, obs)
    std, circ = q.std[:D].copy(), q.circ[:D].copy()
    if mut == "no-wrap":
        circ[len(q.obs) + int(np.argmax(q.circ[len(q.obs):D]))] = False
    if mut == "no-std":
        std[Ds] = 1.0
    y = torch.from_numpy(O.normalize_samples(row, q.mean, std, circ, 0))
    b = torch.from_numpy(np.ascontiguousarray(truncated(q.blob, q.D_model, D, K, H, L), dtype=np.float32))
    lad, outs = torch.zeros_like(y), []
    for lb in O.split_layers(b, D, K, H, L):
        theta = O.layer_theta(y, lb, K, H)
        y, l = O.rqs(y, theta, K, B, inverse=False)
        lad = lad + l
        outs.append(y)
    z, lad = y.numpy(), lad.numpy()
    zp = outs[0].numpy() if mut == "prior-on-first-layer" else z
    logstd = np.log(q.std[:D].astype(np.float32))
    term = lad - np.float32(0.5) * zp * zp - np.float32(HALF_LOG_2PI) - logstd
    acc = np.zeros(X.shape[0], dtype=np.float32)
    widest = Ds + int(np.argmax(np.abs(logstd[Ds:])))       # drop-logstd: the frontal column whose std is furthest from 1
    for i in range(Ds, D):
        acc = acc + (term[:, i] + logstd[i] if (mut == "drop-logstd" and i == widest) else term[:, i])
    if mut == "sep-lad":
        acc = acc + lad[:, Ds - 1]
    if mut == "log2pi-D":
        acc = acc - np.float32(Ds) * np.float32(HALF_LOG_2PI)
    if mut == "half-latent":
        z = z.astype(np.float16).astype(np.float32)
    return acc, z[:, Ds:]


def replay_tree32(name, X, mut=None, only=None):
    K, H, L, total, cliques = walk_tree(name)
    out = [replay_clique32(q, K, H, L, X, mut if only in (None, j) else None) for j, q in enumerate(cliques)]
    return np.stack([p for p, _ in out]), np.concatenate([z.T for _, z in out])


@functools.lru_cache(maxsize=None)
def tree_reference(name):
    """Points, every clique's float64 reference and the float32 replay's outputs and ratios, once per tree (shared)."""
    K, H, L, total, cliques = walk_tree(name)
    X, angle = tree_points(name)
    refs = [clique_scales(q, K, H, L, X) for q in cliques]
    per, lat = replay_tree32(name, X)
    lq = sum_in_table_order(per)
    r_per, r_lat, r_q = tree_ratio(refs, per, lat, lq)
    return dict(X=X, angle=angle, refs=refs, per=per, latent=lat, log_q=lq, R32_per=r_per, R32_lat=r_lat, R32_q=r_q)


def first_rows(refs, n):
    """The references of the first n points (the walk's own draws)."""
    return [dict(r, **{k: r[k][:n] for k in ("t64", "scale", "fwd", "s_z")}) for r in refs]


# ------------------------------------------------------------------ CPU tests: the condition
@pytest.mark.parametrize("name", FORWARD_IDS)
def test_float32_oracle_forward_meets_the_condition(name):
    c, ref = fcase(name), forward_reference(name)
    print("%-16s R32: r_z %6.2f  r_ld %6.2f  r_lp %6.2f" % (name, ref["R32_z"], ref["R32_ld"], ref["R32_lp"]))
    assert max(ref["R32_z"], ref["R32_ld"], ref["R32_lp"]) <= R32_MAX
    assert not exact_failures(ref["x"], ref["z"], ref["ld"], ref["lp"], c.L), exact_failures(ref["x"], ref["z"], ref["ld"], ref["lp"], c.L)
    if c.L == 1:                                           # a tail dim adds exactly 0: the row's log-det is that of the row without it
        x = ref["x"]
        tail = ~(np.abs(x) <= np.float32(B))
        rows = np.where(tail.any(1) & ~tail[:, :-1].any(1))[0] if c.D > 1 else np.where(tail[:, 0])[0]
        assert len(rows) >= 2
        if c.D == 1:
            assert np.all(ref["ld"][rows] == 0.0)
        else:                                              # only the last column is in a tail: nothing conditions on it
            _, ld, _ = oracle_forward(c._replace(D=c.D - 1), x[rows, :-1], blob=truncated(case_blob(c), c.D, c.D - 1, c.K, c.H, c.L))
            assert np.array_equal(_bits(ld), _bits(ref["ld"][rows]))
    for rows in PLACES:                                    # a particle's bits depend neither on n nor on its place
        z, ld, lp = oracle_forward(c, ref["x"][rows])
        assert all(np.array_equal(_bits(a), _bits(b[rows])) for a, b in ((z, ref["z"]), (ld, ref["ld"]), (lp, ref["lp"]))), rows


@pytest.mark.parametrize("name", WALK_TREES)
def test_float32_replay_of_the_tree_terms_meets_the_condition(name):
    ref = tree_reference(name)
    print("%-14s R32 per clique: term %s  latent %s  log_q %.2f" % (name, " ".join("%.2f" % r for r in ref["R32_per"]),
                                                                     " ".join("%.2f" % r for r in ref["R32_lat"]), ref["R32_q"]))
    assert max(ref["R32_per"] + ref["R32_lat"] + [ref["R32_q"]]) <= R32_MAX
    assert np.all(np.isfinite(ref["per"])) and np.all(np.isfinite(ref["latent"]))
    K, H, L, total, cliques = walk_tree(name)
    for j, q in enumerate(cliques):                        # the planted rows are where they were meant to be
        row = clique_row(q, ref["X"]).astype(np.float64)
        D = row.shape[1]
        d = row - q.mean[:D]
        Ds = len(q.obs) + len(q.sep)
        assert np.all(np.abs(np.abs(_wrap(d[:, Ds:][:, q.circ[Ds:D]])) - np.pi) > 0.1)    # frontal angles: away from the seam
        xn = np.where(q.circ[:D], _wrap(d), d) / q.std[:D]
        assert np.sum(np.abs(xn[N:, len(q.obs):]) > B) >= (2 if q.sep else 1)
        if q.circ[len(q.obs):D].any():
            assert np.sum(np.abs(d[:, q.circ[:D]]) > np.pi) >= 20                   # the shifted rows do cross it


def test_the_one_wave_launches_are_above_the_threshold_and_130_points_below():
    for name in ONE_WAVE_TREES:
        nc = len(walk_tree(name)[4])
        assert nc == 3
        assert density_waves(N * ONE_WAVE_COPIES, nc) == (1, 16455)
        assert density_waves(N, nc) == (4, 9)
        assert density_waves(tree_points(name)[0].shape[0], nc)[0] == 4
    assert density_waves(64 * 5461, 3) == (4, 16383) and density_waves(64 * 5461 + 1, 3) == (1, 16386)
    assert density_waves(64 * 16384, 1) == (4, 16384) and density_waves(64 * 16384 + 1, 1) == (1, 16385)


def test_sum_in_table_order_is_the_plain_left_to_right_sum_for_up_to_16_cliques():
    rng = np.random.RandomState(5)
    per = (20 * rng.randn(40, 7)).astype(np.float32)
    for nc in (1, 3, 16):
        s = per[0].copy()
        for c in range(1, nc):
            s = s + per[c]
        assert np.array_equal(_bits(sum_in_table_order(per[:nc])), _bits(s))
    s = [np.float32(0) + per[3 * w] + per[3 * w + 1] + per[3 * w + 2] for w in range(13)] + [np.float32(0) + per[39]]
    t = s[0]
    for v in s[1:]:
        t = t + v
    assert np.array_equal(_bits(sum_in_table_order(per)), _bits(t))


# ------------------------------------------------------------------ CPU tests: the grader -
@pytest.mark.parametrize("name", FORWARD_IDS)
def test_float64_oracle_forward_rounded_to_float32_stays_below_the_float32_oracle(name):
    c, ref = fcase(name), forward_reference(name)
    r_z, r_ld, r_lp = forward_ratio(ref["ref"], *oracle_forward(c, ref["x"], dtype=np.float64))
    print("%-16s float64 oracle rounded: r_z %.2f (R32 %.2f)  r_ld %.2f (R32 %.2f)  r_lp %.2f (R32 %.2f)"
          % (name, r_z.max(), ref["R32_z"], r_ld.max(), ref["R32_ld"], r_lp.max(), ref["R32_lp"]))
    assert r_z.max() <= ref["R32_z"] and r_ld.max() <= ref["R32_ld"] and r_lp.max() <= ref["R32_lp"]


def _neighbouring_bin(x0, init, K):
    """Dim 0 of layer 0 in float64: the point's own left knots, every other quantity (bin sizes, end slopes) of the bin to the
    right -- what a kernel computes that misplaces one knot index -> (z, lad, moved)."""
    th = torch.as_tensor(np.asarray(init), dtype=torch.float64)
    v = torch.as_tensor(x0, dtype=torch.float64)
    cw, wd = O._knots(th[:K], K, B, O.MIN_W)
    ch, ht = O._knots(th[K:2 * K], K, B, O.MIN_H)
    const = math.log(math.exp(1 - O.MIN_D) - 1)
    der = O.MIN_D + torch.nn.functional.softplus(torch.nn.functional.pad(th[2 * K:], (1, 1), value=const))
    k = O._bin(cw.expand(v.shape[0], -1).contiguous(), v).clamp(0, K - 1)
    kn = (k + 1).clamp(0, K - 1)
    xk, yk, dx, dy, d0, d1 = cw[k], ch[k], wd[kn], ht[kn], der[kn], der[kn + 1]
    s = dy / dx
    sig = d0 + d1 - 2 * s
    t = (v - xk) / dx
    q = t * (1 - t)
    den = s + sig * q
    z = yk + dy * (s * t * t + d0 * q) / den
    lad = torch.log(s * s * (d1 * t * t + 2 * s * q + d0 * (1 - t) * (1 - t))) - 2 * torch.log(den)
    return z.numpy(), lad.numpy(), (kn != k).numpy()


@pytest.mark.parametrize("name", [n for n in FORWARD_IDS if fcase(n).L == 1])
def test_the_neighbouring_bins_rational_quadratic_next_to_a_knot_is_flagged(name):
    """L = 1: dim 0's spline output is z[:, 0] and its log-det term a summand of ld.  Every planted point within 2 ulps of a knot,
    one at a time: on the knot or to its right only the log-det shows it, to its left z does as well (see the module docstring)."""
    c, ref = fcase(name), forward_reference(name)
    x, rows = ref["x"], ref["knot_rows"]
    assert len(rows) == 5 * (c.K - 1)
    z0, lad0, moved = _neighbouring_bin(x[rows, 0], case_blob(c)[:3 * c.K - 1], c.K)
    knots = np.repeat(width_knots(case_blob(c)[:3 * c.K - 1], c.K), 5)
    checked = 0
    for j, r in enumerate(rows):
        if not moved[j]:
            continue                                       # the last bin has no neighbour to its right
        z, ld = ref["z"].copy(), ref["ld"].copy()
        z[r, 0] = np.float32(z0[j])
        ld[r] = np.float32(ld[r] - ref["ref"]["lad"][r, 0] + lad0[j])
        r_z, r_ld, _ = forward_ratio(ref["ref"], z, ld)
        if float(x[r, 0]) < knots[j]:
            assert r_z.max() > bound(ref["R32_z"]), (name, r, r_z.max())
        else:
            assert r_ld.max() > bound(ref["R32_ld"]), (name, r, r_ld.max())
        checked += 1
    assert checked >= 5 * (c.K - 1) - 3


def test_the_layer_stride_of_D_where_model_D_was_meant_is_flagged():
    c, ref = fcase("d9l2-D6"), forward_reference("d9l2-D6")
    assert c.model_D == 9 and c.D == 6 and c.L == 2
    full, P = fixture()["blob_d9l2"], O.param_count(6, c.K, c.H)
    z, ld, lp = oracle_forward(c, ref["x"], blob=np.ascontiguousarray(full[:2 * P]))      # layer 1 read P(6) after layer 0
    r_z, r_ld, r_lp = forward_ratio(ref["ref"], z, ld, lp)
    assert r_z.max() > bound(ref["R32_z"]) and r_ld.max() > bound(ref["R32_ld"]) and r_lp.max() > bound(ref["R32_lp"])


def test_dims_8_and_0_swapped_in_the_conditioner_row_are_flagged():
    """D = 9, where wave 0 of eight takes dims 0 and 8: each evaluated with the other's spline parameters."""
    c, ref = fcase("d20h16-D9"), forward_reference("d20h16-D9")
    x = torch.from_numpy(np.nan_to_num(ref["x"], nan=7.5))
    theta = O.layer_theta(x, torch.from_numpy(np.ascontiguousarray(case_blob(c))), c.K, c.H).clone()
    theta[:, [0, 8]] = theta[:, [8, 0]]
    z, lad = O.rqs(x, theta, c.K, B, inverse=False)
    z = np.where(np.isnan(ref["x"]), np.nan, z.numpy()).astype(np.float32)
    ld = lad.sum(1).numpy()
    r_z, r_ld, r_lp = forward_ratio(ref["ref"], z, ld, logprob32(z, ld))
    assert r_z[:, 0].max() > bound(ref["R32_z"]) and r_z[:, 8].max() > bound(ref["R32_z"])
    assert r_z[:, 1:8].max() <= bound(ref["R32_z"])
    assert r_ld.max() > bound(ref["R32_ld"]) and r_lp.max() > bound(ref["R32_lp"])


@pytest.mark.parametrize("name", FORWARD_IDS)
def test_a_float16_rounded_z_and_a_log_det_without_one_dims_term_are_flagged(name):
    c, ref = fcase(name), forward_reference(name)
    z = ref["z"].astype(np.float16).astype(np.float32)
    r_z, _, r_lp = forward_ratio(ref["ref"], z, None, logprob32(z, ref["ld"]))
    assert r_z.max() > bound(ref["R32_z"]) and r_lp.max() > bound(ref["R32_lp"])
    assert np.abs(ref["ref"]["lad"][:, c.D - 1]).max() > 0.05
    ld = (ref["ld"].astype(np.float64) - ref["ref"]["lad"][:, c.D - 1]).astype(np.float32)
    _, r_ld, r_lp = forward_ratio(ref["ref"], None, ld, logprob32(ref["z"], ld))
    assert r_ld.max() > bound(ref["R32_ld"]) and r_lp.max() > bound(ref["R32_lp"])


def _applies(q, mut, L):
    D = len(q.obs) + len(q.sep) + len(q.front)
    return {"sep-lad": bool(q.sep), "drop-logstd": True, "log2pi-D": len(q.obs) + len(q.sep) > 0, "no-std": True,
            "no-wrap": bool(q.circ[len(q.obs):D].any()), "obs-from-point": len(q.obs) > 0, "prior-on-first-layer": L >= 2,
            "half-latent": True}[mut]


TREE_MUTATIONS = ["sep-lad", "drop-logstd", "log2pi-D", "no-wrap", "no-std", "obs-from-point", "prior-on-first-layer", "half-latent"]


@pytest.mark.parametrize("mut", TREE_MUTATIONS)
@pytest.mark.parametrize("name", WALK_TREES)
def test_a_defect_in_one_cliques_term_is_flagged_in_that_clique_alone(name, mut):
    """sep-lad: a separator column's log-det term included; drop-logstd: one frontal column's log std dropped (the one
    with the largest |log std|: a std of 1.0 would make the defect invisible, and rightly so); log2pi-D:
    1/2 log 2 pi counted for D instead of F columns; no-wrap: one angle column not wrapped; no-std: the first frontal column not
    divided by std; obs-from-point: the observation columns read from the point; prior-on-first-layer: the prior of the first
    layer's output (L = 2); half-latent: the latent rounded to float16."""
    K, H, L, total, cliques = walk_tree(name)
    ref = tree_reference(name)
    hit = 0
    for j, q in enumerate(cliques):
        if not _applies(q, mut, L):
            continue
        per, lat = replay_tree32(name, ref["X"], mut, only=j)
        r_per, r_lat, r_q = tree_ratio(ref["refs"], per, lat, sum_in_table_order(per))
        if mut == "half-latent":
            assert r_lat[j] > bound(ref["R32_lat"][j]) and r_per == ref["R32_per"]
        else:
            assert r_per[j] > bound(ref["R32_per"][j]), (name, mut, j, r_per[j])
            assert r_q > bound(ref["R32_q"]), (name, mut, j, r_q)
        assert [r for k, r in enumerate(r_per) if k != j] == [r for k, r in enumerate(ref["R32_per"]) if k != j]
        hit += 1
    assert hit or mut == "prior-on-first-layer" or name.startswith("single")


def test_every_tree_mutation_applies_somewhere():
    for mut in TREE_MUTATIONS:
        assert any(_applies(q, mut, walk_tree(name)[2]) for name in WALK_TREES for q in walk_tree(name)[4]), mut


@pytest.mark.parametrize("name", WALK_TREES)
def test_float64_tree_terms_rounded_to_float32_stay_below_the_float32_replay(name):
    ref = tree_reference(name)
    per = np.stack([r["t64"] for r in ref["refs"]]).astype(np.float32)
    lat = np.concatenate([r["fwd"].T for r in ref["refs"]]).astype(np.float32)
    r_per, r_lat, _ = tree_ratio(ref["refs"], per, lat)
    assert all(a <= b for a, b in zip(r_per + r_lat, ref["R32_per"] + ref["R32_lat"])), (r_per, r_lat)
