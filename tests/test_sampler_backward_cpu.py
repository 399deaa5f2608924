"""Backward error of a posterior draw, element by element, in float64 -- the grader of tests/test_sampler_backward_gpu.py and
its own tests on the CPU.

A sampler (nfisam_nsf_inverse, nfisam_nsf_posterior_walk) returns x = flow^-1(z | given).  Comparing x with another
inverse is loose by construction: the other inverse conditions dim i on ITS x_<i, so a float32 rounding in dim 0 moves every
later dim, and a draw next to a knot may pick the other bin.  Here the sampler's own row [given | drawn] is pushed FORWARD in
float64 (`O.layer_theta`, `O.rqs(..., inverse=False)` per layer) and compared with the latent draw that went in:

    r_z[p, i]  = |fwd64(x)[p, i] - z[p, i]| / (2^-24 L scale),   scale = (B + |z|) + slope (B + |x_n|),  slope = exp(sum_l lad)
    r_ld[p]    = |ld + sum_i lad64[p, i]| / (2^-24 L sum_i (1 + |d lad_i / d x_i| (B + |x_i|)))          (i: drawn dims)

The forward spline is C^1 across knots (either bin will do), dim i is judged with the sampler's x_<i (no chain), the tails are
the identity (exact).  `scale` is what half an ulp of the quantities of size <= B + |.| on either side of the spline moves z
by; `d lad_i / d x_i` is autograd's, with the conditioning held fixed.  With `norm = (mean, std, circular)` the sampler's RAW
row is normalised again in float64 (angle columns: wrap(x - mean) / std; an angle outside [-pi, pi] counts as residual) and
slope (|x_raw| + |mean| + pi circular) / std joins `scale`: the rounding of the un-normalisation.

The bound is not fixed here: every case also runs the project's float32 oracle (`CO.inverse(dtype=float32)`, with
`O.normalize_samples` / `O.unnormalize_samples` around it) through the same grader.  Its largest ratio is R32;
    condition on the inputs   R32 <= 64             (the reference alone behaves: trained-like parameters only)
    bound on a sampler        max r <= 8 max(R32, 4) over EVERY element -- no quantile, no mask.
The factor 8: the device's exp2 / log2 / rcp are 1-ulp instructions, its tanh = 1 - 2 rcp(1 + exp2(.)) has an absolute error of
a few 2^-24 per activation where libm's is relative, and its sums are FMA chains in another order.

Measured on the float32 oracle (B = 5, n = 130; the MI355X's figures are in profiles/sampler_backward_error.json): R32 of r_z
1.8 .. 4.9 at L = 1 and for the trained flows, up to 8.5 at L = 2 (D = 12, H = 16); of r_ld 0.7 .. 5.6; of the walk 1.2 .. 3.7 per
clique.  `test_float32_oracle_meets_the_condition` prints every case's.

Two choices the wrapped output forces: an angle column's std is at most 0.4 (7.5 std < pi, so that wrap(x_raw - mean) / std IS
the normalised value the kernel had; a wider column's wrapped draw does not determine it), and the walk's latent draws carry no
NaN (a NaN frontal column would be every descendant's separator; `nfisam_nsf_inverse` gets one, in its last column).

The CPU tests below grade the grader: mutations of the float32 oracle's output that a wrong kernel would produce (a shifted
column, swapped columns, the neighbouring bin's rational-quadratic, a wrong slope logit at the box edge, a missing wrap, the
reference's literal multi-layer conditioning, a dropped log-det term) must each exceed the bound."""
import functools
import math
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import c_oracle as CO
from oracle import nsf_torch as O

EPS32 = 2.0 ** -24
B = 5.0
N = 130                      # two full 64-tiles and a partial one (four and a partial 32-tile of the two-lane walk)
R32_MAX = 64.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_flows.npz")
BOUND_LOGIT = math.log(math.exp(1 - O.MIN_D) - 1)


def bound(r32):
    return 8.0 * max(float(r32), 4.0)


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def truncated(blob, model_D, D, K, H, L):
    """The first D dims of a model_D-dim autoregressive flow are its D-dim marginal flow: the first param_count(D) of every layer."""
    if model_D == D:
        return blob
    Pt, P = O.param_count(D, K, H), O.param_count(model_D, K, H)
    return np.concatenate([blob[l * P:l * P + Pt] for l in range(L)])


# ------------------------------------------------------------------ the grader -----------
def _wrap(t):
    return (t + np.pi) % (2 * np.pi) - np.pi


def forward64(xn, blob, K, H, L):
    """Normalised rows xn [n, D] -> (fwd [n, D], lad [n, D] summed over layers, d lad_i / d x_i [n, D]) in float64.  Every layer's
    conditioning is held fixed in the derivative (theta is computed from detached inputs), so autograd returns the diagonal."""
    D = xn.shape[1]
    b = torch.as_tensor(np.asarray(blob), dtype=torch.float64)
    x0 = torch.as_tensor(xn, dtype=torch.float64).clone().requires_grad_(True)
    y, lad = x0, torch.zeros_like(x0)
    for lb in O.split_layers(b, D, K, H, L):
        theta = O.layer_theta(y.detach(), lb, K, H)
        y, l = O.rqs(y, theta, K, B, inverse=False)
        lad = lad + l
    (g,) = torch.autograd.grad(lad.sum(), x0)
    return y.detach().numpy(), lad.detach().numpy(), g.numpy()


def backward_ratio(x_full32, z, blob, K, H, B_, L, Ds, norm=None, ld=None):
    """x_full32 [n, D]: the sampler's row [given | drawn] (raw units when `norm` is given, else normalised); z [n, D - Ds] the latent
    draws; blob: torch-layout parameters of the D-dim flow.  -> (r_z [n, D - Ds], r_ld [n] or None).  A NaN draw that comes back NaN
    has ratio 0 (its bits are the caller's to compare); any other non-finite value has ratio inf."""
    assert B_ == B
    x = np.asarray(x_full32, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    n, D = x.shape
    assert z.shape == (n, D - Ds)
    extra, excess = np.zeros((n, D)), np.zeros((n, D))
    xn = x
    if norm is not None:
        mean, std, circ = (np.asarray(a)[:D] for a in norm)
        mean, std, circ = mean.astype(np.float64), std.astype(np.float64), circ.astype(bool)
        d = x - mean
        xn = np.where(circ, _wrap(d), d) / std
        extra = (np.abs(x) + np.abs(mean) + np.pi * circ) / std
        excess = np.where(circ, np.maximum(np.abs(x) - np.pi, 0.0), 0.0) / std
    nan_pair = np.isnan(z) & np.isnan(xn[:, Ds:])
    xe = xn.copy()
    xe[:, Ds:][nan_pair] = 2 * B                         # a tail value: identity, log-det 0, conditions nothing here
    extra[:, Ds:][nan_pair] = 0.0
    excess[:, Ds:][nan_pair] = 0.0
    fwd, lad, dlad = forward64(xe, blob, K, H, L)
    ze = np.where(nan_pair, 2 * B, z)
    slope = np.exp(lad[:, Ds:])
    xa = np.abs(xe[:, Ds:])
    res = np.abs(fwd[:, Ds:] - ze) + slope * excess[:, Ds:]
    scale = (B + np.abs(ze)) + slope * (B + xa + extra[:, Ds:])
    r_z = res / (EPS32 * L * scale)
    r_z = np.where(np.isfinite(r_z), r_z, np.inf)
    r_ld = None
    if ld is not None:
        s = (1.0 + np.abs(dlad[:, Ds:]) * (B + xa + extra[:, Ds:])).sum(1)
        r_ld = np.abs(np.asarray(ld, dtype=np.float64) + lad[:, Ds:].sum(1)) / (EPS32 * L * s)
        r_ld = np.where(np.isfinite(r_ld), r_ld, np.inf)
    return r_z, r_ld


def exact_failures(xhat, z, ld=None):
    """The tolerance-free properties of a normalised-space draw (mean == NULL) -> list of messages (empty: all hold).
    |z| > B or NaN: the bits of z come back; everything else is finite and stays in the box."""
    xhat, z = np.asarray(xhat, dtype=np.float32), np.asarray(z, dtype=np.float32)
    tail = ~(np.abs(z) <= np.float32(B))
    bad = []
    if not np.array_equal(xhat.view(np.int32)[tail], z.view(np.int32)[tail]):
        bad.append("a tail / NaN draw did not come back with its own bits")
    if not np.all(np.isfinite(xhat[~tail])):
        bad.append("non-finite draw inside the box")
    elif not np.all(np.abs(xhat[~tail]) <= np.float32(B)):
        bad.append("|x| > B for |z| <= B: max excess %.3g" % (np.abs(xhat[~tail]).max() - B))
    if ld is not None and not np.all(np.isfinite(ld)):
        bad.append("non-finite log-det")
    return bad


# ------------------------------------------------------------------ the cases ------------
# nfisam_nsf_inverse: (name, blob, model_D, D, Ds, norm).  K, H, L come with the blob.
Case = namedtuple("Case", "name blob model_D D Ds K H L norm seed")
_INVERSE = [("d1", 1, 0), ("d5", 5, 0), ("d12", 12, 3), ("d5k2", 5, 0), ("d5k16", 5, 0), ("d20h16", 20, 0), ("d12k5h4", 12, 4),
            ("d5l2", 5, 0), ("d7l2", 7, 3), ("d7l3", 7, 1), ("d12h16l2", 12, 3),
            ("trained3", 3, 0), ("trained3", 3, 1), ("trained4", 4, 0), ("trained4", 4, 1),
            ("d9l2", 6, 2)]                                               # model_D = 9 > D = 6: the layer stride
_NORMED = [("d12", 12, 3), ("d7l2", 7, 3)]


def _shape(key):
    fx = fixture()
    if key.startswith("trained"):
        D, K, H, L = (int(v) for v in fx["shape_" + key][:4])
    else:
        D, K, H, L = (int(v) for v in fx["recipe_shapes"][list(fx["recipe_names"]).index(key)][:4])
    return D, K, H, L


def inverse_cases():
    out = []
    for j, (key, D, Ds) in enumerate(_INVERSE):
        mD, K, H, L = _shape(key)
        out.append(Case("%s-D%d-Ds%d" % (key, D, Ds), key, mD, D, Ds, K, H, L, False, 1000 + j))
    for j, (key, D, Ds) in enumerate(_NORMED):
        mD, K, H, L = _shape(key)
        out.append(Case("%s-D%d-Ds%d-normed" % (key, D, Ds), key, mD, D, Ds, K, H, L, True, 2000 + j))
    return out


INVERSE_CASES = inverse_cases()
CASE_IDS = [c.name for c in INVERSE_CASES]


def case_blob(c):
    return truncated(fixture()["blob_" + c.blob], c.model_D, c.D, c.K, c.H, c.L)


def case_norm(c):
    """mean, std in [0.3, 1.5], circular over the D dims: one given and one drawn angle column; the drawn one has mean 3.0, so that
    outputs cross the +-pi seam, and std 0.4 (7.5 std < pi: the wrapped output still determines the normalised value)."""
    if not c.norm:
        return None
    rng = np.random.RandomState(c.seed + 7)
    mean = (2 * rng.randn(c.D)).astype(np.float32)
    std = (0.3 + 1.2 * rng.rand(c.D)).astype(np.float32)
    circ = np.zeros(c.D, dtype=bool)
    g, d = c.Ds - 1, c.Ds + 1
    circ[[g, d]] = True
    mean[g], std[g] = -2.5, 0.9
    mean[d], std[d] = 3.0, 0.4
    return mean, std, circ


def height_knots(init_param, K):
    """Interior knots of the height spline of a shared theta, in float64."""
    th = torch.as_tensor(np.asarray(init_param), dtype=torch.float64)
    ch, _ = O._knots(th[K:2 * K], K, B, O.MIN_H)
    return ch.numpy()[1:-1]


SPECIALS = [B, -B, np.nextafter(np.float32(B), np.float32(0)), np.nextafter(np.float32(B), np.float32(9)),
            np.nextafter(np.float32(-B), np.float32(0)), np.nextafter(np.float32(-B), np.float32(-9)),
            7.5, -7.5, np.nan, 0.0, -4.9999]


def case_inputs(c):
    """-> (z [N, F] float32, given [N, Ds] float32 or None; raw units for a normed case).  z = 1.3 randn with planted rows: the box
    edges, both float32 neighbours of each, +-7.5 and NaN (tails), 0 and -4.9999 -- once counted from the first drawn column and
    once from the last, NaN always in the last (nothing is conditioned on it) -- and, for dim 0 of an unconditioned flow, the
    float32 values at and 1, 2 ulps around every interior height knot of the layer that consumes z."""
    rng = np.random.RandomState(c.seed)
    F = c.D - c.Ds
    z = (1.3 * rng.randn(N, F)).astype(np.float32)
    row = 0
    for rev in (False, True):
        for j, v in enumerate(SPECIALS):
            col = F - 1 if np.isnan(v) else (F - 1 - j % F if rev else j % F)
            z[row, col] = v
            row += 1
    if c.Ds == 0:
        P = O.param_count(c.D, c.K, c.H)
        init = case_blob(c)[(c.L - 1) * P:(c.L - 1) * P + 3 * c.K - 1]
        for y in height_knots(init, c.K):
            v = np.float32(y)
            lo1, hi1 = np.nextafter(v, np.float32(-9)), np.nextafter(v, np.float32(9))
            for u in (np.nextafter(lo1, np.float32(-9)), lo1, v, hi1, np.nextafter(hi1, np.float32(9))):
                z[row, 0] = u
                row += 1
    assert row <= N - 20
    given = None
    if c.Ds:
        given = (1.2 * rng.randn(N, c.Ds)).astype(np.float32)
        given[0, 0], given[1, c.Ds - 1] = 5.5, -5.0                       # a given column in the tail / on the box edge
        if c.norm:
            mean, std, circ = case_norm(c)
            given = (given * std[:c.Ds] + mean[:c.Ds]).astype(np.float32)
            given[:, circ[:c.Ds]] = _wrap(given[:, circ[:c.Ds]].astype(np.float64)).astype(np.float32)
    return z, given


def oracle_inverse(c, z, given, dtype=np.float32, blob=None):
    """The project's oracle on the case -> (row [given | drawn] float32, raw units for a normed case; ld)."""
    blob = case_blob(c) if blob is None else blob
    norm = case_norm(c)
    g = given
    if norm is not None and c.Ds:
        g = O.normalize_samples(given, *norm, 0)
    xf, ld = CO.inverse(z, g, blob, c.K, c.H, B, c.L, dtype=dtype)
    xf = xf.astype(np.float32)
    if norm is not None:
        xf = O.unnormalize_samples(xf, *norm, c.Ds)
    return (np.concatenate([given, xf], 1) if c.Ds else xf), ld


def grade(c, row, z, ld=None):
    return backward_ratio(row, z, case_blob(c), c.K, c.H, B, c.L, c.Ds, norm=case_norm(c), ld=ld)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, the float32 oracle's row and its ratios, computed once per case and shared (callers must not modify them)."""
    c = INVERSE_CASES[CASE_IDS.index(name)]
    z, given = case_inputs(c)
    row, ld = oracle_inverse(c, z, given)
    r_z, r_ld = grade(c, row, z, ld)
    return dict(z=z, given=given, row=row, ld=ld, R32_z=float(r_z.max()), R32_ld=float(r_ld.max()))


# ------------------------------------------------------------------ the walk's trees -----
Clique = namedtuple("Clique", "blob mean std circ D_model obs sep front")
WALK_TREES = ["tree-l1h8", "tree-l1h16", "tree-l1h4", "tree-l2h8", "single-d19h16", "single-d20h16"]


def walk_tree(name):
    """-> (K, H, L, total, [Clique]).  The three-clique tree is `_walk_tree_problem` of tests/test_hip_parity.py: root {v0, v1} ->
    child {v2 | v1} -> leaf {v3 | v2, part of v0}, sample-matrix columns permuted, one model larger than used.  Angle columns
    have std in [0.3, 0.4] (see case_norm).  The single-clique trees sit just below and just above the LDS switch of the
    two-lane walk (H = 16: max_D = 19 fits 150 KB, 20 does not; `walk2_lds_bytes`)."""
    fx = fixture()
    K = 9
    if name.startswith("single"):
        key = "walk_" + name[7:]
        D, _, H, L = _shape(key)
        specs = [dict(n_obs=2, sep=[], front=list(np.random.RandomState(D).permutation(D - 2)))]
        keys, total = [key], D - 2
    else:
        L, H = int(name[6]), int(name[8:])
        specs = [dict(n_obs=0, sep=[], front=[4, 5, 6, 7, 8]), dict(n_obs=2, sep=[7, 8], front=[1, 2, 3]),
                 dict(n_obs=1, sep=[1, 2, 3, 4, 5], front=[0])]
        keys, total = ["walk_l%dh%d_c%d" % (L, H, j) for j in range(3)], 9
    rng = np.random.RandomState(sum(map(ord, name)))
    cliques = []
    for sp, key in zip(specs, keys):
        D = _shape(key)[0]
        mean = (2 * rng.randn(D)).astype(np.float32)
        std = (0.5 + rng.rand(D)).astype(np.float32)
        circ = rng.rand(D) < 0.3
        std[circ] = (0.3 + 0.1 * rng.rand(int(circ.sum()))).astype(np.float32)
        obs = rng.randn(sp["n_obs"]).astype(np.float32)
        cliques.append(Clique(fx["blob_" + key], mean, std, circ, D, obs, [int(v) for v in sp["sep"]], [int(v) for v in sp["front"]]))
    return K, H, L, total, cliques


def walk_latents(name, total):
    """Zt [total, N] float32: 1.3 randn, the SPECIALS planted along the first rows of every latent row's column range."""
    rng = np.random.RandomState(sum(map(ord, name)) + 1)
    Zt = (1.3 * rng.randn(total, N)).astype(np.float32)
    for r in range(total):
        for j, v in enumerate(SPECIALS):
            if not np.isnan(v):
                Zt[r, (r * 3 + j * 7) % N] = v
    return Zt


def walk2_lds_bytes(max_D, K, H, L, kparam_count):
    """LDS of the two-lane walk (`unit_walk`): two parameter buffers of the widest clique, its constants, columns and tiles."""
    return (2 * L * kparam_count(max_D, K, H) + 8 * max_D + 2 * max_D + 3 * max_D * 34) * 4


def oracle_walk(name, Zt, dtype=np.float32):
    """FactorGraphSolver.sample_posterior with the oracle, as `_oracle_walk` of tests/test_hip_parity.py slices it, in float32:
    normalise the given columns, conditional inverse of the truncated flow, un-normalise -> S [N, total] float32."""
    K, H, L, total, cliques = walk_tree(name)
    S = np.zeros((N, total), dtype=np.float32)
    zrow = 0
    for q in cliques:
        Ds, F = len(q.obs) + len(q.sep), len(q.front)
        xs_n = None
        if Ds:
            given = np.concatenate([np.tile(q.obs, (N, 1)), S[:, q.sep]], 1).astype(np.float32)
            xs_n = O.normalize_samples(given, q.mean, q.std, q.circ, 0)
        tb = truncated(q.blob, q.D_model, Ds + F, K, H, L)
        xf, _ = CO.inverse(Zt[zrow:zrow + F].T, xs_n, tb, K, H, B, L, dtype=dtype)
        zrow += F
        S[:, q.front] = O.unnormalize_samples(xf.astype(np.float32), q.mean, q.std, q.circ, Ds)
    return S


def grade_walk(name, S, Zt):
    """One `backward_ratio` call per clique: the model truncated to its first Ds + F dims, Zt rows in walk order, the given
    columns taken from the graded sample matrix itself -> [largest r_z per clique]."""
    K, H, L, total, cliques = walk_tree(name)
    S = np.asarray(S, dtype=np.float32)
    out, zrow = [], 0
    for q in cliques:
        Ds, F = len(q.obs) + len(q.sep), len(q.front)
        row = np.concatenate([np.tile(q.obs, (N, 1)), S[:, q.sep], S[:, q.front]], 1)
        r_z, _ = backward_ratio(row, Zt[zrow:zrow + F].T, truncated(q.blob, q.D_model, Ds + F, K, H, L), K, H, B, L, Ds,
                                norm=(q.mean, q.std, q.circ))
        zrow += F
        out.append(float(r_z.max()))
    return out


@functools.lru_cache(maxsize=None)
def walk_reference(name):
    K, H, L, total, cliques = walk_tree(name)
    Zt = walk_latents(name, total)
    S = oracle_walk(name, Zt)
    return dict(Zt=Zt, S=S, R32=grade_walk(name, S, Zt))


# ------------------------------------------------------------------ CPU tests ------------
def _c(name):
    return INVERSE_CASES[CASE_IDS.index(name)]


@pytest.mark.parametrize("name", CASE_IDS)
def test_float32_oracle_meets_the_condition(name):
    c, ref = _c(name), reference(name)
    print("%-24s R32: r_z %6.2f  r_ld %6.2f" % (name, ref["R32_z"], ref["R32_ld"]))
    assert ref["R32_z"] <= R32_MAX and ref["R32_ld"] <= R32_MAX
    if not c.norm:
        z = ref["z"]
        tail = ~(np.abs(z) <= B)
        assert np.array_equal(ref["row"][:, c.Ds:].view(np.int32)[tail], z.view(np.int32)[tail])
        assert np.all(np.isfinite(ref["row"][:, c.Ds:][~tail])) and np.all(np.isfinite(ref["ld"]))


@pytest.mark.parametrize("name", WALK_TREES)
def test_float32_oracle_walk_meets_the_condition(name):
    ref = walk_reference(name)
    print("%-16s R32 per clique: %s" % (name, " ".join("%.2f" % r for r in ref["R32"])))
    assert max(ref["R32"]) <= R32_MAX


@pytest.mark.parametrize("name", CASE_IDS)
def test_float64_oracle_rounded_to_float32_stays_below_the_float32_oracle(name):
    c, ref = _c(name), reference(name)
    row, ld = oracle_inverse(c, ref["z"], ref["given"], dtype=np.float64)
    r_z, r_ld = grade(c, row, ref["z"], ld.astype(np.float32))
    print("%-24s float64 oracle rounded: r_z %.2f (R32 %.2f)  r_ld %.2f (R32 %.2f)"
          % (name, r_z.max(), ref["R32_z"], r_ld.max(), ref["R32_ld"]))
    assert r_z.max() <= ref["R32_z"] and r_ld.max() <= ref["R32_ld"]


def _flagged(c, ref, row, ld=None):
    r_z, r_ld = grade(c, row, ref["z"], ld)
    over_z = r_z.max() > bound(ref["R32_z"])
    over_ld = ld is not None and r_ld.max() > bound(ref["R32_ld"])
    return over_z, over_ld, float(r_z.max())


# A shift dx of one column moves z by slope dx: r = slope dx / (2^-24 L scale).  With scale <= (B + 7.5) (1 + slope) a row of
# slope >= 1 reads AT LEAST 1e-4 / (2^-24 L 25) = 67 / L, which alone clears the bound of every L = 1 case; most rows read far
# more (scale is nearer 2 B than 25, and a later column also sees the shifted one through its conditioner), and the shift is
# flagged in every case, L = 2 and 3 included (the tightest: the last column at L = 3, about 80 against a bound of 36).
@pytest.mark.parametrize("name", CASE_IDS)
def test_a_shift_of_1e_4_in_one_drawn_column_is_flagged(name):
    c, ref = _c(name), reference(name)
    if c.L == 1:
        assert bound(ref["R32_z"]) < 67.0
    for col in sorted({c.Ds, c.D - 1}):
        row = ref["row"].copy()
        row[:, col] += np.float32(1e-4)
        assert _flagged(c, ref, row)[0], (name, col)


@pytest.mark.parametrize("name", [n for n in CASE_IDS if _c(n).D - _c(n).Ds >= 2])
def test_two_swapped_drawn_columns_are_flagged(name):
    c, ref = _c(name), reference(name)
    row = ref["row"].copy()
    row[:, [c.Ds, c.Ds + 1]] = row[:, [c.Ds + 1, c.Ds]]
    assert _flagged(c, ref, row)[0]


def _inverse_in_neighbouring_bin(z, init, K):
    """Dim 0 of an unconditioned layer, in float64: the draw's own left knots, every other quantity (bin sizes, end slopes) of the
    bin to the right -- what a kernel computes that misplaces one knot index."""
    th = torch.as_tensor(np.asarray(init), dtype=torch.float64)
    v = torch.as_tensor(z, dtype=torch.float64)
    cw, wd = O._knots(th[:K], K, B, O.MIN_W)
    ch, ht = O._knots(th[K:2 * K], K, B, O.MIN_H)
    der = O.MIN_D + torch.nn.functional.softplus(torch.nn.functional.pad(th[2 * K:], (1, 1), value=BOUND_LOGIT))
    k = O._bin(ch.expand(v.shape[0], -1).contiguous(), v).clamp(0, K - 1)
    kn = (k + 1).clamp(0, K - 1)
    xk, yk, dx, dy, d0, d1 = cw[k], ch[k], wd[kn], ht[kn], der[kn], der[kn + 1]
    s = dy / dx
    sig = d0 + d1 - 2 * s
    dlt = v - yk
    a, b, cc = dlt * sig + dy * (s - d0), dy * d0 - dlt * sig, -s * dlt
    t = (2 * cc) / (-b - torch.sqrt(b * b - 4 * a * cc))
    return (t * dx + xk).numpy(), (kn != k).numpy()


@pytest.mark.parametrize("name", [n for n in CASE_IDS if _c(n).Ds == 0 and _c(n).L == 1])
def test_the_neighbouring_bins_rational_quadratic_is_flagged(name):
    """On the cases whose dim 0 has a shared theta and whose spline output is the draw itself (Ds = 0, L = 1): there the mutated
    value can be written into the oracle's row without running a conditioner or a further layer on it."""
    c, ref = _c(name), reference(name)
    z = ref["z"]
    inside = np.abs(z[:, 0]) <= B
    x0, moved = _inverse_in_neighbouring_bin(np.where(inside, z[:, 0], 0.0), case_blob(c)[:3 * c.K - 1], c.K)
    rows = np.where(inside & moved)[0][:3]                                 # a few percent of the samples
    assert len(rows) == 3
    row = ref["row"].copy()
    row[rows, 0] = x0[rows].astype(np.float32)
    assert _flagged(c, ref, row)[0]


@pytest.mark.parametrize("name", CASE_IDS)
def test_a_wrong_last_slope_logit_at_the_box_edge_is_flagged(name):
    """The last interior slope logit of every drawn dim (layer L - 1) read as its neighbour in the padded row, the padding
    constant: only draws inside the last two bins move (not those on a knot or on the box edge)."""
    c, ref = _c(name), reference(name)
    blob = torch.from_numpy(case_blob(c).copy())
    Po = 3 * c.K - 1
    init, nets = O.unpack(O.split_layers(blob, c.D, c.K, c.H, c.L)[c.L - 1], c.D, c.K, c.H)      # views into `blob`
    for i in range(c.Ds, c.D):
        if i == 0:
            init[Po - 1] = BOUND_LOGIT
        else:
            nets[i - 1][4][Po - 1, :] = 0.0
            nets[i - 1][5][Po - 1] = BOUND_LOGIT
    row, _ = oracle_inverse(c, ref["z"], ref["given"], blob=blob.numpy())
    assert not np.array_equal(row, ref["row"])
    assert _flagged(c, ref, row)[0]


@pytest.mark.parametrize("name", [n for n in CASE_IDS if _c(n).norm])
def test_an_unnormalisation_without_the_wrap_is_flagged(name):
    c, ref = _c(name), reference(name)
    mean, std, circ = case_norm(c)
    g = O.normalize_samples(ref["given"], mean, std, circ, 0)
    xf, _ = CO.inverse(ref["z"], g, case_blob(c), c.K, c.H, B, c.L, dtype=np.float32)
    raw = O.unnormalize_samples(xf, mean, std, np.zeros(c.D, dtype=bool), c.Ds)
    assert np.sum(np.abs(raw[:, circ[c.Ds:]]) > np.pi) >= 10                # outputs do cross the seam
    row = np.concatenate([ref["given"], raw], 1)
    assert _flagged(c, ref, row)[0]
    assert np.all(np.abs(ref["row"][:, c.Ds:][:, circ[c.Ds:]]) <= np.float32(np.pi))


@pytest.mark.parametrize("name", [n for n in CASE_IDS if _c(n).L >= 2 and _c(n).Ds > 0])
def test_the_references_literal_multilayer_conditioning_is_flagged(name):
    """Every layer conditioned on the same (normalised) given columns, the reference's loop: inverts no composition."""
    c, ref = _c(name), reference(name)
    norm = case_norm(c)
    b = torch.as_tensor(case_blob(c), dtype=torch.float64)
    xs = torch.as_tensor(ref["given"] if norm is None else O.normalize_samples(ref["given"], *norm, 0), dtype=torch.float64)
    x = torch.as_tensor(np.nan_to_num(ref["z"], nan=7.5), dtype=torch.float64)
    for lb in reversed(O.split_layers(b, c.D, c.K, c.H, c.L)):
        x, _ = O.layer_inverse(x, lb, c.K, c.H, B, x_sep=xs, D=c.D)
    xf = np.where(np.isnan(ref["z"]), np.nan, x.numpy()).astype(np.float32)
    if norm is not None:
        xf = O.unnormalize_samples(xf, *norm, c.Ds)
    row = np.concatenate([ref["given"], xf], 1)
    assert _flagged(c, ref, row)[0]


@pytest.mark.parametrize("name", CASE_IDS)
def test_a_log_det_without_one_dims_term_is_flagged(name):
    c, ref = _c(name), reference(name)
    norm = case_norm(c)
    xn = ref["row"].astype(np.float64)
    if norm is not None:
        xn = O.normalize_samples(ref["row"], *norm, 0).astype(np.float64)
    _, lad, _ = forward64(np.nan_to_num(xn, nan=7.5), case_blob(c), c.K, c.H, c.L)
    ld = (ref["ld"].astype(np.float64) + lad[:, c.D - 1]).astype(np.float32)           # ld = -sum lad: the last dim's term gone
    assert np.abs(lad[:, c.D - 1]).max() > 0.05
    over_z, over_ld, _ = _flagged(c, ref, ref["row"], ld)
    assert over_ld and not over_z


def test_walk_grader_flags_a_shifted_column_and_a_clique_fed_another_cliques_separator():
    name = "tree-l1h8"
    ref = walk_reference(name)
    K, H, L, total, cliques = walk_tree(name)
    S = ref["S"].copy()
    S[:, cliques[2].front[0]] += np.float32(1e-4) * cliques[2].std[-1]
    r = grade_walk(name, S, ref["Zt"])
    assert r[2] > bound(ref["R32"][2]) and r[:2] == ref["R32"][:2]
    S = ref["S"].copy()
    S[:, [7, 8]] = S[:, [8, 7]]                                            # the child's separator columns swapped after the fact
    r = grade_walk(name, S, ref["Zt"])
    assert r[0] > bound(ref["R32"][0]) and r[1] > bound(ref["R32"][1])
