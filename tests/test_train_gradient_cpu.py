"""The training gradient graded per parameter against float64 -- the grader of tests/test_train_gradient_gpu.py, its cases, the
conditions on them and its own tests on the CPU.

tests/test_hip_parity.py holds the gradient to rtol 1e-3 + atol 2e-5 max|ref|: an absolute term of the LARGEST entry, on a sum
over particles, mostly between forms that could share an error.  Here every entry is graded on its own scale, in float64:

    g64, gx64   CO.nll_grad / CO.backward with dtype = float64 on the float32 inputs (the cast is exact); NLL mode: the mean over n
    S_j         sum_p |g64 of particle p alone|_j     one oracle call per row x[p:p+1] (/ n in NLL mode): the condition of the sum
    T_j         the largest S over the parameter tensor of j (per layer: init_param; per dim W0, b0, W1, b1, W2, b2): a floor for
                entries that cancel inside one particle
    sigma_j     the largest |g64(x~, th~) - g64|_j over 32 seeded perturbations x~ = x (1 + 2^-24 xi), th~ = th (1 + 2^-24 xi'),
                xi uniform in [-1, 1], in float64: what an input rounding alone does -- the gradient's own conditioning, the
                finite jump of the log-det term's theta-gradient when a particle crosses a knot included
    scale_j     2^-24 (S_j + T_j) + sigma_j                              r_j = |g_j - g64_j| / scale_j
    dL/dx       scale[p, i] = 2^-24 (|gx64[p, i]| + max_i' |gx64[p, i']| + |gz[p, i]| + |gl[p]|) + sigma_x[p, i]
                (NLL mode: gz = z64 / n, gl = -1 / n, what the oracle feeds its own backward pass)
    loss        |loss - loss64| / (2^-24 mean_p |log p64(x_p)| (depth + 2)),  depth = (L + 1) D + 6 + ceil(n / 32)
                additions on the path of one particle's term to the sum: D squares and L D log-det terms are chained, a
                64-lane sum takes 6 steps, and every tile (32 particles in the finest form) adds its sum to the clique's --
                one after the other in the worst case (atomics).  Each rounds at most 2^-24 of a partial sum, which the mean
                |log p| bounds per particle; + 2: the division by n and the constant D/2 log 2 pi.

The bound is not fixed here: every case also runs the project's float32 oracle through the grader; its largest ratio is R32,
separately for the parameters, dL/dx and the loss.
    condition on the inputs   R32 <= 32
    condition on the scale    the share of parameters with sigma_j > 64 2^-24 (S_j + T_j) is at most 1 %: else knot crossings
                              could excuse too much
    bound on a device form    max r <= 8 max(R32, 4) over EVERY parameter and EVERY dL/dx element -- no quantile, no mask.
Factor 8 and floor 4 are those of tests/test_sampler_backward_cpu.py, for the same reasons: the device's exp2 / log2 / rcp are
1-ulp instructions, its tanh = 1 - 2 rcp(1 + exp2(.)) has an absolute error, its sums are FMA chains in another order.  Seeds
and cases are chosen so that both conditions hold for the reference alone; a case that misses one is replaced, not admitted.

Cases (B = 5; n = 130: two 64-tiles and a partial one; parameters and x as `make_problem` of tests/test_hip_parity.py makes
them -- reference initialisation + 0.25 noise, x = 1.6 randn, the rows x = 5.5, -5.0, 5.0, 4.9999 it places kept):
    L = 1       (D, K, H) = (5,9,8) (12,9,8) (5,16,8) (5,2,8) (12,5,4) (20,9,16) (1,9,8) (100,9,8: past the dim-major limit)
    L > 1       (7,9,8,3) (12,9,16,2) (6,9,4,2), (4,9,8,2) at n = 1
    n           (5,9,8,1) at n = 1, 33, 64, 65
    trained     trained3 / trained4 of tests/golden/sampler_flows.npz with the first 130 rows of their own data
    tails       column 0 wholly outside [-B, B]: the gradient of layer 0's init_param is EXACTLY 0 (no tolerance)
    knots       VJP with gz = randn, gl = 0 on (5,9,8,1) and (4,16,16,1): rows on every interior width-knot of dim 0 and of the
                last dim (float64 knots of `O.layer_theta` / `O._knots`, rounded to float32).  z is C^1 in theta across a knot, so
                either bin is right; the log-det term is not, hence gl = 0.  In EVERY OTHER case no particle lies within
                2^-20 B of an interior float64 knot of its own spline in any layer (asserted)
    vjp         gz, gl = randn, one case per (K, H) above
    ragged      (n, D) = (33,12) (65,1) (1,4) and (130,5) at K = 9, H = 8, L = 1 and 2 (one TrainBatch on the GPU)
    atomic      129 tiles of 64 and of 32 particles at D = 2, K = 5: past the slab limit, the reduction is under test
Saturated parameters are OUT OF SCOPE: with noise >= 3 on the logits the float32 oracle's own ratio is 1e3 .. 1e4 -- the
reference is then no yardstick (the likely reason two earlier attempts at "knots, tails and saturated parameters" held no bound).

Measured on the float32 oracle (`test_float32_oracle_meets_both_conditions` prints every case's): R32 of the parameters 0.5 .. 9.4,
22.8 for the single particle at L = 2; of dL/dx 0.7 .. 19.1; of the loss below 0.4 (the oracle sums it in double); sigma-share at
most 0.92 % (the VJP case at D = 20, H = 16).  An MI355X's ratios are in profiles/train_gradient_error.json.

The CPU tests below grade the grader.  Mutations of the float32 oracle's output that a wrong kernel would produce must each
exceed the bound: a dropped particle, a particle counted twice, the last 2 particles dropped (the partial tile), an n / (n + 1)
scaling, two neighbouring b2 entries swapped, the last dim's W2 rounded through float16, one particle's contribution scaled
by 1 + 1e-3, one particle's log-det term taken from the neighbouring bin (L = 1, dim 0: there the term can be restated without
running a conditioner or a further layer on it), a W0 column of dim i taken from dim i - 1, dL/dx of one row shifted by one
column, the gl term omitted from dL/dx."""
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
N = 130
R32_MAX = 32.0
SIGMA_FACTOR, SIGMA_SHARE_MAX = 64.0, 0.01
N_PERTURB = 32
KNOT_CLEARANCE = 2.0 ** -20 * B
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_flows.npz")
BOUND_LOGIT = math.log(math.exp(1 - O.MIN_D) - 1)
SLAB_MAX_TILES = 128                     # NFISAM_SLAB_MAX_TILES' default: more tiles than this and the gradient goes through atomics


def bound(r32):
    return 8.0 * max(float(r32), 4.0)


def loss_depth(n, D, L):
    return (L + 1) * D + 6 + -(-n // 32)


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in ("blob_trained3", "x_trained3", "shape_trained3", "blob_trained4", "x_trained4", "shape_trained4")}


# ------------------------------------------------------------------ the cases ------------
Case = namedtuple("Case", "name kind n D K H L seed")


def _name(kind, n, D, K, H, L):
    return "%s-n%d-d%dk%dh%dl%d" % (kind, n, D, K, H, L)


def _cases():
    out = []

    def add(kind, n, D, K, H, L, seed=None, name=None):
        name = name or _name(kind, n, D, K, H, L)
        if name not in [c.name for c in out]:
            out.append(Case(name, kind, n, D, K, H, L, 7000 + len(out) if seed is None else seed))
    for D, K, H in [(5, 9, 8), (12, 9, 8), (5, 16, 8), (5, 2, 8), (12, 5, 4), (20, 9, 16), (1, 9, 8), (100, 9, 8)]:
        add("nll", N, D, K, H, 1)
    for D, K, H, L, n in [(7, 9, 8, 3, N), (12, 9, 16, 2, N), (6, 9, 4, 2, N), (4, 9, 8, 2, 1)]:
        # (12,9,16,2): the seed in line (7009) has a sigma-share of 2.4 %, as have 7100 and 7104 (4.6 - 5.1 %); 7101 - 7103, 7105 - 7107: <= 0.2 %
        add("nll", n, D, K, H, L, seed=7101 if (D, H) == (12, 16) else None)
    for n in (1, 33, 64, 65):
        add("nll", n, 5, 9, 8, 1)
    for key in ("trained3", "trained4"):
        D, K, H, L = (int(v) for v in fixture()["shape_" + key][:4])
        add("trained", N, D, K, H, L, name=key)
    add("tails", N, 5, 9, 8, 1)
    add("tails", N, 6, 9, 4, 2)
    add("knots", N, 5, 9, 8, 1)
    add("knots", N, 4, 16, 16, 1)
    for D, K, H, L in [(5, 9, 8, 1), (5, 16, 8, 1), (5, 2, 8, 1), (12, 5, 4, 1), (20, 9, 16, 1), (6, 9, 4, 2)]:
        add("vjp", N, D, K, H, L)
    for L in (1, 2):                                                     # the ragged batch; some are cases above already
        for n, D in RAGGED:
            add("nll", n, D, 9, 8, L)
    add("nll", (SLAB_MAX_TILES + 1) * 64, 2, 5, 8, 1, name="atomic64")
    add("nll", (SLAB_MAX_TILES + 1) * 32, 2, 5, 8, 1, name="atomic32")
    return out


RAGGED = [(130, 5), (33, 12), (65, 1), (1, 4)]
CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def case(name):
    return CASES[CASE_IDS.index(name)]


def ragged_names(L):
    return [_name("nll", n, D, 9, 8, L) for n, D in RAGGED]


def make_problem(n, D, K, H, L, seed, spread=1.6):
    """`make_problem` of tests/test_hip_parity.py: reference initialisation + 0.25 noise, x = spread randn, four placed rows."""
    gen = torch.Generator().manual_seed(seed)
    blob = torch.cat([O.init_blob(D, K, H, gen) for _ in range(L)])
    blob = blob + 0.25 * torch.randn(blob.shape, generator=gen)
    x = spread * torch.randn(n, D, generator=gen)
    for r, (c, v) in enumerate([(0, 5.5), (D - 1, -5.0), (D // 2, 5.0), (0, 4.9999)]):
        if r < n:
            x[r, c] = v
    return blob.numpy().astype(np.float32), x.numpy().astype(np.float32)


def layer_inputs64(x, blob, K, H, L):
    """-> [(y [n, D] the layer's input, interior width-knots [n, D, K - 1]) per layer], float64 torch."""
    D = x.shape[1]
    b = torch.from_numpy(np.array(blob, dtype=np.float64))
    y = torch.from_numpy(np.array(x, dtype=np.float64))
    out = []
    for lb in O.split_layers(b, D, K, H, L):
        theta = O.layer_theta(y, lb, K, H)
        cw, _ = O._knots(theta[..., :K], K, B, O.MIN_W)
        out.append((y, cw[..., 1:-1]))
        y, _ = O.rqs(y, theta, K, B, inverse=False)
    return out


def knot_distance(x, blob, K, H, L):
    """The smallest distance of any particle's coordinate to an interior float64 knot of its own spline, over all layers."""
    if K < 2:
        return np.inf
    return min(float((y[..., None] - kn).abs().min()) for y, kn in layer_inputs64(x, blob, K, H, L))


KNOT_ROW0 = 4                                                            # behind the rows `make_problem` places


def plant_knots(x, blob, K, H):
    """Rows on every interior width-knot of dim 0 and of the last dim (L = 1), float64 knots rounded to float32 -> planted (row, dim)."""
    D = x.shape[1]
    planted, row = [], KNOT_ROW0
    for dim in (0, D - 1):
        for k in range(K - 1):
            (y, kn), = layer_inputs64(x[row:row + 1], blob, K, H, 1)       # the last dim's knots depend on the row's x_<D-1 only
            x[row, dim] = np.float32(float(kn[0, dim, k]))
            planted.append((row, dim))
            row += 1
    assert row <= x.shape[0]
    return planted


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(x [n, D] float32, blob float32 torch layout, gz [n, D] / gl [n] float32 or None for the NLL mode, planted)."""
    c = case(name)
    planted = []
    if c.kind == "trained":
        blob, x = fixture()["blob_" + name].copy(), np.ascontiguousarray(fixture()["x_" + name][:c.n])
    else:
        blob, x = make_problem(c.n, c.D, c.K, c.H, c.L, c.seed)
    rng = np.random.RandomState(c.seed)
    gz = gl = None
    if c.kind == "tails":
        x[:, 0] = (np.where(rng.rand(c.n) < 0.5, -1.0, 1.0) * (B + 0.01 + np.abs(rng.randn(c.n)))).astype(np.float32)
        x[0, 0], x[1, 0] = np.nextafter(np.float32(B), np.float32(9)), np.nextafter(np.float32(-B), np.float32(-9))
    if c.kind in ("vjp", "knots"):
        gz = rng.randn(c.n, c.D).astype(np.float32)
        gl = np.zeros(c.n, dtype=np.float32) if c.kind == "knots" else rng.randn(c.n).astype(np.float32)
    if c.kind == "knots":
        planted = plant_knots(x, blob, c.K, c.H)
    for a in (x, blob, gz, gl):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, blob=blob, gz=gz, gl=gl, planted=planted)


# ------------------------------------------------------------------ the grader -----------
def param_tensors(D, K, H, L):
    """-> (tensor id per parameter [L P], {(layer, dim, name): slice}) in the torch layout; dim 0 holds init_param only."""
    Po, P = 3 * K - 1, O.param_count(D, K, H)
    tid, where, t = np.empty(L * P, dtype=np.int64), {}, 0
    for l in range(L):
        off = l * P
        for i in range(D):
            parts = [("init_param", Po)] if i == 0 else [("W0", H * i), ("b0", H), ("W1", H * H), ("b1", H), ("W2", Po * H), ("b2", Po)]
            for nm, cnt in parts:
                where[(l, i, nm)] = slice(off, off + cnt)
                tid[off:off + cnt] = t
                off, t = off + cnt, t + 1
        assert off == (l + 1) * P
    return tid, where


def oracle_grad(c, x, blob, gz, gl, dtype, want_loss=False):
    """The oracle's gradient in the case's mode -> (g [L P], gx [n, D], loss or None, logprob [n] or None); NLL: the mean over n."""
    if gz is None:
        loss, g, lp, gx = CO.nll_grad(x, blob, c.K, c.H, B, c.L, dtype=dtype, want_gx=True)
        return g, gx, loss, lp
    g, gx = CO.backward(x, blob, gz, gl, c.K, c.H, B, c.L, dtype=dtype)
    return g, gx, None, None


def particle_grad(c, inp, p, dtype=np.float64):
    """Particle p's term of the case's gradient: the oracle on the row x[p:p+1] alone (/ n in NLL mode)."""
    if inp["gz"] is None:
        return CO.nll_grad(inp["x"][p:p + 1], inp["blob"], c.K, c.H, B, c.L, dtype=dtype)[1] / np.dtype(dtype).type(c.n)
    return CO.backward(inp["x"][p:p + 1], inp["blob"], inp["gz"][p:p + 1], inp["gl"][p:p + 1], c.K, c.H, B, c.L, dtype=dtype)[0]


def _ratio(err, scale):
    """err / scale; 0 where both are 0 (an entry that is exactly 0 and must be), inf where only the scale is."""
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    r = np.divide(err, scale, out=np.zeros_like(err), where=scale > 0)
    r = np.where((scale <= 0) & (err > 0), np.inf, r)
    return np.where(np.isfinite(err), r, np.inf)


def param_ratio(g, ref, extra=None):
    """r_j of a gradient g [L P] in the torch layout; `extra` [L P] joins the scale (a documented, derived term only)."""
    scale = ref["scale"] if extra is None else ref["scale"] + extra
    return _ratio(np.abs(np.asarray(g, dtype=np.float64) - ref["g64"]), scale)


def gx_ratio(gx, ref):
    return _ratio(np.abs(np.asarray(gx, dtype=np.float64) - ref["gx64"]), ref["scale_x"])


def loss_ratio(loss, ref):
    return float(_ratio(abs(float(loss) - ref["loss64"]), ref["scale_loss"]))


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the grader needs for a case, computed once and shared (callers must not modify it): the float64 gradient, its
    scales, and the float32 oracle's gradient with its ratios."""
    c, inp = case(name), inputs(name)
    x, blob, gz, gl = inp["x"], inp["blob"], inp["gz"], inp["gl"]
    g64, gx64, loss64, lp64 = oracle_grad(c, x, blob, gz, gl, np.float64)
    tid, where = param_tensors(c.D, c.K, c.H, c.L)
    S = np.zeros_like(g64)
    for p in range(c.n):
        S += np.abs(particle_grad(c, inp, p))
    tmax = np.zeros(tid.max() + 1)
    np.maximum.at(tmax, tid, S)
    T = tmax[tid]
    sigma, sigma_x = np.zeros_like(g64), np.zeros_like(gx64)
    rng = np.random.RandomState(c.seed + 99)
    x64, b64 = x.astype(np.float64), blob.astype(np.float64)
    for _ in range(N_PERTURB):
        xp = x64 * (1 + EPS32 * rng.uniform(-1, 1, x64.shape))
        bp = b64 * (1 + EPS32 * rng.uniform(-1, 1, b64.shape))
        gp, gxp, _, _ = oracle_grad(c, xp, bp, gz, gl, np.float64)
        np.maximum(sigma, np.abs(gp - g64), out=sigma)
        np.maximum(sigma_x, np.abs(gxp - gx64), out=sigma_x)
    base = EPS32 * (S + T)
    if gz is None:
        z64, _ = CO.forward(x, blob, c.K, c.H, B, c.L, dtype=np.float64)
        up_z, up_l = np.abs(z64) / c.n, np.full(c.n, 1.0 / c.n)
    else:
        up_z, up_l = np.abs(gz.astype(np.float64)), np.abs(gl.astype(np.float64))
    scale_x = EPS32 * (np.abs(gx64) + np.abs(gx64).max(1, keepdims=True) + up_z + up_l[:, None]) + sigma_x
    ref = dict(g64=g64, gx64=gx64, loss64=loss64, S=S, T=T, sigma=sigma, sigma_x=sigma_x, scale=base + sigma, scale_x=scale_x,
               sigma_share=float(np.mean(sigma > SIGMA_FACTOR * base)), tid=tid, where=where)
    if gz is None:
        ref["scale_loss"] = EPS32 * float(np.mean(np.abs(lp64))) * (loss_depth(c.n, c.D, c.L) + 2)
    g32, gx32, loss32, _ = oracle_grad(c, x, blob, gz, gl, np.float32)
    ref.update(g32=g32, gx32=gx32, loss32=loss32, R32=float(param_ratio(g32, ref).max()), R32_x=float(gx_ratio(gx32, ref).max()),
               R32_loss=loss_ratio(loss32, ref) if gz is None else 0.0)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def exceeds(name, g=None, gx=None):
    """Does the mutated gradient (or dL/dx) exceed the case's bound?  -> (flag, largest ratio, bound)"""
    ref = reference(name)
    if g is not None:
        r, b = float(param_ratio(g, ref).max()), bound(ref["R32"])
    else:
        r, b = float(gx_ratio(gx, ref).max()), bound(ref["R32_x"])
    return r > b, r, b


# ------------------------------------------------------------------ CPU tests ------------
SMALL = [n for n in CASE_IDS if case(n).n <= N]                          # the mutation tests leave the two atomic-sink cases out
SUMMED = [n for n in SMALL if case(n).n >= 33]                           # a sum over particles to go wrong in


@pytest.mark.parametrize("name", CASE_IDS)
def test_float32_oracle_meets_both_conditions(name):
    c, ref = case(name), reference(name)
    print("%-24s R32: parameters %6.2f  dL/dx %6.2f  loss %5.2f   sigma-share %.4f"
          % (name, ref["R32"], ref["R32_x"], ref["R32_loss"], ref["sigma_share"]))
    assert ref["R32"] <= R32_MAX and ref["R32_x"] <= R32_MAX and ref["R32_loss"] <= R32_MAX
    assert ref["sigma_share"] <= SIGMA_SHARE_MAX


@pytest.mark.parametrize("name", CASE_IDS)
def test_particles_keep_clear_of_interior_knots_except_where_planted(name):
    c, inp = case(name), inputs(name)
    if c.kind != "knots":
        assert knot_distance(inp["x"], inp["blob"], c.K, c.H, c.L) > KNOT_CLEARANCE
        return
    (y, kn), = layer_inputs64(inp["x"], inp["blob"], c.K, c.H, c.L)
    assert len(inp["planted"]) == 2 * (c.K - 1)
    for j, (row, dim) in enumerate(inp["planted"]):
        assert abs(float(y[row, dim] - kn[row, dim, j % (c.K - 1)])) <= EPS32 * B        # half an ulp of a value below B
    assert np.all(inp["gl"] == 0)


@pytest.mark.parametrize("name", [n for n in CASE_IDS if case(n).kind == "tails"])
def test_a_column_in_the_tails_leaves_layer_0s_init_param_without_gradient(name):
    c, inp, ref = case(name), inputs(name), reference(name)
    assert np.all(np.abs(inp["x"][:, 0]) > np.float32(B))
    sl = ref["where"][(0, 0, "init_param")]
    assert np.all(ref["g64"][sl] == 0) and np.all(ref["g32"][sl] == 0) and np.all(ref["scale"][sl] == 0)
    assert np.abs(ref["g64"]).max() > 0
    g = ref["g32"].copy()
    g[sl.start + 3] = np.float32(1e-30)                                    # anything but 0 there is infinitely wrong
    assert exceeds(name, g=g)[0]


@pytest.mark.parametrize("name", SMALL)
def test_float64_oracle_rounded_to_float32_stays_below_the_float32_oracle(name):
    ref = reference(name)
    assert param_ratio(ref["g64"].astype(np.float32), ref).max() <= max(ref["R32"], 1.0)
    assert gx_ratio(ref["gx64"].astype(np.float32), ref).max() <= max(ref["R32_x"], 1.0)


@functools.lru_cache(maxsize=None)
def _particle_shares(name):
    """-> (the particle whose own term is the largest share of some parameter's S + T, the particle with the median of that figure:
    a particle like any other).  A placed row may have no term at all in a one-dim flow (x = 5.5: the identity), hence no fixed row."""
    c, inp, ref = case(name), inputs(name), reference(name)
    share = np.array([np.max(np.abs(particle_grad(c, inp, p)) / np.maximum(ref["S"] + ref["T"], 1e-300)) for p in range(c.n)])
    order = np.argsort(-share)
    return int(order[0]), int(order[len(order) // 2])


def _largest_particle(name):
    return _particle_shares(name)[0]


def _typical_particle(name):
    return _particle_shares(name)[1]


@pytest.mark.parametrize("name", SUMMED)
def test_a_dropped_and_a_doubled_particle_are_flagged(name):
    c, inp, ref = case(name), inputs(name), reference(name)
    for p in sorted({_typical_particle(name), c.n // 2, c.n - 1}):
        t = particle_grad(c, inp, p, np.float32)
        for sign in (-1, 1):
            flag, r, b = exceeds(name, g=ref["g32"] + sign * t)
            assert flag, (name, p, sign, r, b)


@pytest.mark.parametrize("name", SUMMED)
def test_a_dropped_partial_tile_is_flagged(name):
    c, inp, ref = case(name), inputs(name), reference(name)
    g = ref["g32"] - particle_grad(c, inp, c.n - 1, np.float32) - particle_grad(c, inp, c.n - 2, np.float32)
    assert exceeds(name, g=g)[0]


@pytest.mark.parametrize("name", [n for n in SMALL if case(n).kind not in ("vjp", "knots")])       # the NLL mode's mean
def test_a_mean_over_n_plus_1_is_flagged(name):
    c, ref = case(name), reference(name)
    s = np.float32(c.n) / np.float32(c.n + 1)
    assert exceeds(name, g=ref["g32"] * s)[0]
    assert exceeds(name, gx=ref["gx32"] * s)[0]


def _last_dim_tensor(c, ref, nm):
    """The last dim's `nm` of the last layer; a one-dim flow has only init_param, which is its b2 and W2 alike."""
    return ref["where"][(c.L - 1, c.D - 1, nm if c.D > 1 else "init_param")]


@pytest.mark.parametrize("name", SMALL)
def test_two_swapped_neighbouring_b2_entries_are_flagged(name):
    c, ref = case(name), reference(name)
    sl = _last_dim_tensor(c, ref, "b2")
    # a pair of width, of height and of slope logits; the slopes next to an empty bin have no gradient at all (both 0 at n = 1
    # but for the particle's own bin: no swap to see), so theirs is the pair whose float64 entries differ most
    slopes = ref["g64"][sl][2 * c.K:]
    for o in (0, c.K) + ((2 * c.K + int(np.argmax(np.abs(np.diff(slopes)))),) if len(slopes) >= 2 else ()):
        g = ref["g32"].copy()
        g[[sl.start + o, sl.start + o + 1]] = g[[sl.start + o + 1, sl.start + o]]
        flag, r, b = exceeds(name, g=g)
        assert flag, (name, o, r, b)


@pytest.mark.parametrize("name", SMALL)
def test_the_last_dims_w2_rounded_through_float16_is_flagged(name):
    c, ref = case(name), reference(name)
    sl = _last_dim_tensor(c, ref, "W2")
    g = ref["g32"].copy()
    g[sl] = g[sl].astype(np.float16).astype(np.float32)
    assert exceeds(name, g=g)[0]


@pytest.mark.parametrize("name", SMALL)
def test_one_particle_off_by_1e_3_relative_is_flagged(name):
    c, inp, ref = case(name), inputs(name), reference(name)
    for p in sorted({_largest_particle(name), _typical_particle(name)}):     # (measured: the largest reads 3 .. 190 x the bound, the typical one from 1.5 x)
        g = ref["g32"] + np.float32(1e-3) * particle_grad(c, inp, p, np.float32)
        flag, r, b = exceeds(name, g=g)
        assert flag, (name, p, r, b)


def _lad_dim0(v, theta, K, shift):
    """log |dz/dx| of dim 0 (shared theta [3K - 1], float64) at the scalar v, by the rational-quadratic of the bin `shift` bins
    from v's own (`O.rqs` restated for one element with the bin index moved) -> (lad, own bin, t in the own bin)."""
    cw, wd = O._knots(theta[:K], K, B, O.MIN_W)
    _, ht = O._knots(theta[K:2 * K], K, B, O.MIN_H)
    der = O.MIN_D + torch.nn.functional.softplus(torch.nn.functional.pad(theta[2 * K:], (1, 1), value=BOUND_LOGIT))
    k0 = int(O._bin(cw, v).clamp(0, K - 1))
    k = min(max(k0 + shift, 0), K - 1)
    s = ht[k] / wd[k]
    t = (v - cw[k]) / wd[k]
    q = t * (1 - t)
    den = s + (der[k] + der[k + 1] - 2 * s) * q
    num = s * s * (der[k + 1] * t * t + 2 * s * q + der[k] * (1 - t) * (1 - t))
    return torch.log(num) - 2 * torch.log(den), k0, float(((v - cw[k0]) / wd[k0]).detach())


def _dlad_dtheta(v, init, K, shift):
    th = torch.from_numpy(np.array(init, dtype=np.float64)).requires_grad_(True)
    lad, k0, t0 = _lad_dim0(torch.tensor(float(v), dtype=torch.float64), th, K, shift)
    (g,) = torch.autograd.grad(lad, th)
    return g.numpy(), k0, t0


@pytest.mark.parametrize("name", [n for n in SMALL if case(n).L == 1 and case(n).kind in ("nll", "trained") and case(n).n >= 33 and case(n).K > 2])
def test_one_particles_log_det_term_from_the_neighbouring_bin_is_flagged(name):
    """NLL mode, L = 1: init_param reaches the loss through z_0 and lad_0 only, so particle p's term of its gradient is
    (z_0 dz_0/dtheta - dlad_0/dtheta) / n and the log-det part can be exchanged on its own.  The particle is the one nearest a
    knot of dim 0 (relative to its bin), the neighbour the bin across that knot: the mildest such error."""
    c, inp, ref = case(name), inputs(name), reference(name)
    init = inp["blob"][:3 * c.K - 1]
    best = None
    for p in range(c.n):
        v = float(inp["x"][p, 0])
        if abs(v) >= B:
            continue
        _, k0, t0 = _dlad_dtheta(v, init, c.K, 0)
        shift = -1 if t0 < 0.5 else 1
        if 0 <= k0 + shift < c.K and (best is None or min(t0, 1 - t0) < best[0]):
            best = (min(t0, 1 - t0), p, shift)
    _, p, shift = best
    own, _, _ = _dlad_dtheta(inp["x"][p, 0], init, c.K, 0)
    other, _, _ = _dlad_dtheta(inp["x"][p, 0], init, c.K, shift)
    assert np.all(np.isfinite(other)) and np.abs(other - own).max() > 0
    g = ref["g32"].copy()
    sl = ref["where"][(0, 0, "init_param")]
    g[sl] = (g[sl].astype(np.float64) + (own - other) / c.n).astype(np.float32)         # the gradient of -lad: the own bin's out, the other's in
    flag, r, b = exceeds(name, g=g)
    assert flag, (name, p, shift, r, b)
    # the restated term is the oracle's: with it taken out altogether, particle p's init_param term is z_0 dz_0/dtheta alone
    th = torch.from_numpy(np.array(init, dtype=np.float64)).requires_grad_(True)
    z, _ = O.rqs(torch.tensor([float(inp["x"][p, 0])], dtype=torch.float64), th[None, :], c.K, B)
    (gz0,) = torch.autograd.grad(0.5 * (z * z).sum(), th)
    np.testing.assert_allclose((gz0.numpy() - own) / c.n, particle_grad(c, inp, p)[sl], rtol=1e-9, atol=1e-14)


@pytest.mark.parametrize("name", [n for n in SMALL if case(n).D >= 3])
def test_a_w0_column_taken_from_the_dim_before_is_flagged(name):
    c, ref = case(name), reference(name)
    i = c.D - 1
    a, b_ = ref["where"][(c.L - 1, i, "W0")], ref["where"][(c.L - 1, i - 1, "W0")]
    g = ref["g32"].copy()
    W, Wprev = g[a].reshape(c.H, i), ref["g32"][b_].reshape(c.H, i - 1)
    W[:, 0] = Wprev[:, 0]
    g[a] = W.reshape(-1)
    assert exceeds(name, g=g)[0]


@pytest.mark.parametrize("name", [n for n in SMALL if case(n).D >= 2])
def test_dl_dx_of_one_row_shifted_by_one_column_is_flagged(name):
    c, ref = case(name), reference(name)
    for p in sorted({0, c.n // 2, c.n - 1}):
        gx = ref["gx32"].copy()
        gx[p] = np.roll(gx[p], 1)
        assert exceeds(name, gx=gx)[0], (name, p)


@pytest.mark.parametrize("name", [n for n in SMALL if case(n).kind != "knots"])
def test_dl_dx_without_the_gl_term_is_flagged(name):
    c, inp, ref = case(name), inputs(name), reference(name)
    if inp["gz"] is None:
        z32, _ = CO.forward(inp["x"], inp["blob"], c.K, c.H, B, c.L, dtype=np.float32)
        gz = z32 / np.float32(c.n)
    else:
        gz = inp["gz"]
    _, gx = CO.backward(inp["x"], inp["blob"], gz, np.zeros(c.n, dtype=np.float32), c.K, c.H, B, c.L, dtype=np.float32)
    assert exceeds(name, gx=gx)[0]


def test_the_grader_takes_the_float32_oracles_own_output_and_the_tensor_map_is_the_layouts():
    ref = reference(CASE_IDS[0])
    c = case(CASE_IDS[0])
    assert not exceeds(c.name, g=ref["g32"])[0] and not exceeds(c.name, gx=ref["gx32"])[0]
    tid, where = param_tensors(c.D, c.K, c.H, c.L)
    init, nets = O.unpack(torch.arange(O.param_count(c.D, c.K, c.H)), c.D, c.K, c.H)
    assert where[(0, 0, "init_param")] == slice(int(init[0]), int(init[-1]) + 1)
    for i, net in enumerate(nets, start=1):
        for nm, t in zip(("W0", "b0", "W1", "b1", "W2", "b2"), net):
            assert where[(0, i, nm)] == slice(int(t.reshape(-1)[0]), int(t.reshape(-1)[-1]) + 1)
            assert len(set(tid[where[(0, i, nm)]])) == 1
