"""`nfisam_simulate_clique` (csrc/clique_sim.hip) replayed sample by sample in float64, and `nfisam_normalize_columns`
against a float64 oracle.

The simulator is deterministic: Philox4x32-10 keyed by the clique's seed, counter (sample, op index), Box-Muller, then
SE(2) / R2 algebra in float32.  `oracle/clique_sim_ref.py` rebuilds the uniforms bit for bit, so every mixture pick is
exact and every output a smooth function of known inputs: every sample of every test is compared, none is left out.
The schedules and their tolerance |dev - f64| <= 4 E_c + 2^-23 max|column c| are built in tests/test_clique_sim_cpu.py (E_c:
the float64 replay against the same formulas in numpy float32, column by column).  Measured E_c, translations / headings,
and as information the largest share of the tolerance an MI355X used (every check prints it):

  raw draws (four seeds) 9.9e-6 / 9.6e-7, 0.27      every op, inputs to +-50 m 1.8e-5 / 1.6e-6, 0.31
  small heading noise 2.8e-6 / 8.6e-7, 0.27         scratch columns, n = 1 .. 600 2.5e-6 / 3.2e-7, 0.23
  wide launches 1.3e-5 / 7.6e-7, 0.25               40 ops 3.8e-6, 0.29
  the eight-factor clique 4.5e-6 / 3.5e-7, 0.26

Normalisation: the kernel sums in double and rounds once, so mean and std are held to 2 float32 ulps of the oracle
and x_out to 2 ulps + 1e-7.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import clique_sim_ref as R
from test_clique_sim_cpu import (HEADING_NOISE, MIX_W, SEEDS, SHAPE_N, WIDE_D, all_ops_case, cached, case, col_diff,
                                 eight_factor_set, forty_ops_case, raw_draws_case, rec, reference, scratch_case,
                                 small_heading_case, wide_case)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7777.0


def upload_sources(cs, n=None):
    return {k: torch.from_numpy(np.ascontiguousarray(v[:n])).to(DEV) for k, v in cs["sources"].items()}


def device_ops(cs, n=None, keep=None):
    """The case's records as `nfisam_hip.SimOp`s; a COPY's src becomes the pointer of the uploaded (first n rows of the)
    source -> (ops, tensors to keep alive)."""
    import nfisam_hip as nh
    keep = upload_sources(cs, n) if keep is None else keep
    ops = []
    for r in cs["ops"]:
        o = nh.SimOp()
        o.code, o.a, o.b, o.c, o.k = r.code, r.a, r.b, r.c, r.k
        o.src = keep[r.src].data_ptr() if r.code == R.COPY else 0
        for i, v in enumerate(r.p):
            o.p[i] = v
        for i, v in enumerate(r.cand):
            o.cand[i] = v
        ops.append(o)
    return ops, keep


def launch(cs, n=None):
    import nfisam_hip as nh
    ops, keep = device_ops(cs, n)
    out = nh.simulate_clique(ops, n or cs["n"], cs["D_out"], cs["D_total"], cs["seed"], DEV).cpu().numpy()
    del keep
    return out


def launch_into(buf, ops, n, D_out, D_total, seed):
    """The C entry on a buffer of the test's own -> return code."""
    import nfisam_hip as nh
    arr = (nh.SimOp * len(ops))(*ops)
    rc = nh.lib().nfisam_simulate_clique(arr, len(ops), int(n), int(D_out), int(D_total), C.c_uint64(int(seed)),
                                         nh._ptr(buf), nh._stream())
    torch.cuda.synchronize()
    return rc


def check(name, out, ref, angles):
    """Every sample of every column inside the tolerance; prints what share of it the device used."""
    r64, tol, E = ref
    assert out.shape == r64.shape and out.dtype == np.float32 and np.all(np.isfinite(out))
    d = col_diff(out, r64, angles)
    share = (d / np.where(tol > 0, tol, 1.0)).max()
    in_E = (np.maximum(d.max(0) - 2.0 ** -23 * np.abs(r64).max(0), 0) / np.where(E > 0, E, np.inf)).max()
    print("%-34s device / tolerance %.2f   (device - one ulp) / E_c %.2f" % (name, share, in_E))
    bad = np.argwhere(d > tol)
    assert bad.size == 0, (name, len(bad), bad[:5], d[tuple(bad[0])], tol[bad[0][1]])


# ---- the generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_raw_draws_equal_the_replay(seed):
    """(z0, z1), wrap(z2), the bearing's (cos, sin) and both null-hypothesis picks, exposed by ops with unit parameters,
    under seeds with an empty and a full upper key word; n = 600 is blocks of 256, 256 and 88 samples."""
    cs, ref = cached(raw_draws_case, seed)
    out = launch(cs)
    check(cs["name"], out, ref, cs["angles"])
    n, w = cs["n"], np.float32(MIX_W)
    z64 = R._Arith(np.float64)
    # which sigma the samples took: |value| / |z0| is 1 or 10
    u5, u6 = R.uniforms(seed, n, 5), R.uniforms(seed, n, 6)
    z5, z6 = z64.draw(u5)[0], z64.draw(u6)[0]
    assert min(np.abs(z5).min(), np.abs(z6).min()) > 1e-5
    dev_obs = np.abs(out[:, 11].astype(np.float64) / z5) < np.sqrt(10.0)
    dev_ring = np.linalg.norm(out[:, 12:14].astype(np.float64) - cs["sources"][1], axis=1) / np.abs(z6) < np.sqrt(10.0)
    np.testing.assert_array_equal(dev_obs, u5[2] < w)                      # NH_OBS picks with u2
    np.testing.assert_array_equal(dev_ring, u6[3] < w)                     # NH_RING picks with u3
    assert 0.6 < dev_obs.mean() < 0.8 and 0.6 < dev_ring.mean() < 0.8
    # the bearing is (2 u2 - 1) pi of the op's own counter
    phi = np.arctan2(out[:, 10].astype(np.float64), out[:, 9].astype(np.float64))
    dphi = np.abs((phi - z64.bearing(R.uniforms(seed, n, 4)[2]) + np.pi) % (2 * np.pi) - np.pi)
    assert dphi.max() < 1e-6, dphi.max()


def test_streams_are_per_op_index_and_per_sample():
    """The same op at two indices of one list draws differently, each as its own replay says; sample q draws the same at
    every n (the first 300 rows of an n = 600 run are the n = 300 run, bit for bit); a second call gives the same bits."""
    raw2, raw3 = [0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 1]
    cs = case("one op at two indices", [rec(R.PRIOR_R2, c=0, p=raw2), rec(R.PRIOR_R2, c=2, p=raw2),
                                         rec(R.PRIOR_SE2, c=4, p=raw3), rec(R.PRIOR_SE2, c=7, p=raw3)], 600, 10, 10,
              2 ** 62 - 1, angles=[6, 9])
    out = launch(cs)
    check(cs["name"], out, reference(cs), cs["angles"])
    assert not np.any(out[:, 0:2] == out[:, 2:4]) and not np.any(out[:, 6] == out[:, 9])
    cs, _ = cached(raw_draws_case, SEEDS[2])
    whole, again, half = launch(cs), launch(cs), launch(cs, n=300)
    assert whole.tobytes() == again.tobytes()
    assert half.shape == (300, cs["D_out"]) and whole[:300].tobytes() == half.tobytes()


# ---- every op, per sample --------------------------------------------------------------------------------------------------
def test_every_op_with_noise_equals_the_replay():
    """One schedule with all 15 codes: copied poses and points to +-50 m with headings over [-pi, pi), full Cholesky factors,
    three REL_FWD chained, a REL_BWD, a REL_OBS over both ends, a 3-way and a 4-way ADA_OBS with unequal weights."""
    cs, ref = cached(all_ops_case)
    out = launch(cs)
    check(cs["name"], out, ref, cs["angles"])
    np.testing.assert_array_equal(out[:, :12], cs["sources"][1])
    # the association ops really spread over their candidates (replayed picks, exact)
    for o, k, cum in ((9, 3, [0.2, 0.7]), (10, 4, [0.1, 0.5, 0.8])):
        u2 = R.uniforms(cs["seed"], cs["n"], o)[2]
        pick = np.searchsorted(np.array(cum, dtype=np.float32), u2, side="right")
        assert sorted(set(pick)) == list(range(k))


@pytest.mark.parametrize("l22", HEADING_NOISE)
def test_small_heading_noise_equals_the_replay(l22):
    """PRIOR_SE2 / REL_FWD / REL_BWD / REL_OBS with 1 m of translation noise and heading noise down to 0: the exponential
    map's b = (1 - cos w) / w for |w| from 1e-8 to 1e-2, both sides of its series branch.  (The float32-cancelling form
    misses this bound by a factor of 45-64: tests/test_clique_sim_cpu.py::test_cancelling_exp_map_misses_the_bound.)"""
    cs, ref = cached(small_heading_case, l22)
    check(cs["name"], launch(cs), ref, cs["angles"])


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPE_N)
def test_partial_blocks_with_scratch_columns(n):
    """n around the 256-sample block with D_out < D_total: the n x D_out output is fully written (it equals the replay)
    and the row allocated behind it is untouched."""
    cs, ref = cached(scratch_case, n)
    ops, _ = device_ops(cs)
    buf = torch.full((n + 1, cs["D_out"]), SENTINEL, dtype=torch.float32, device=DEV)
    assert launch_into(buf, ops, n, cs["D_out"], cs["D_total"], cs["seed"]) == 0
    got = buf.cpu().numpy()
    check(cs["name"], got[:n], ref, cs["angles"])
    assert np.all(got[n] == np.float32(SENTINEL))


@pytest.mark.parametrize("D_total", WIDE_D)
def test_wide_launches_on_both_sides_of_48_kb(D_total):
    """D_total KB of dynamic LDS: 48 is the last size the plain launch takes, from 49 on the entry raises the kernel's limit
    first; 150 is the cap."""
    cs, ref = cached(wide_case, D_total)
    out = launch(cs)
    check(cs["name"], out, ref, cs["angles"])
    np.testing.assert_array_equal(out[:, :D_total - 10], cs["sources"][1])


def test_limits_of_columns_and_ops():
    import nfisam_hip as nh
    cs, ref = cached(forty_ops_case)
    check(cs["name"], launch(cs), ref, cs["angles"])
    ops, _ = device_ops(cs)
    with pytest.raises(ValueError):
        nh.simulate_clique(ops + ops[:1], cs["n"], cs["D_out"], cs["D_total"], cs["seed"], DEV)        # 41 ops
    with pytest.raises(ValueError):
        nh.simulate_clique(ops, cs["n"], cs["D_out"], 151, cs["seed"], DEV)
    buf = torch.full((cs["n"], cs["D_out"]), SENTINEL, dtype=torch.float32, device=DEV)
    assert launch_into(buf, ops, cs["n"], cs["D_out"], 151, cs["seed"]) == nh.ERR_ARG
    assert bool((buf == SENTINEL).all())


# ---- through the compiler --------------------------------------------------------------------------------------------------
def test_compiled_clique_equals_the_replay_of_its_own_launch(monkeypatch):
    """The eight-factor clique through `FusedSimulationBackend`: the launch it compiles (recorded on the way) replayed on
    the host ties the real factors' Cholesky factors, cumulative weights and column plan to the kernel, per sample."""
    import nfisam_hip as nh
    from sampler.DeviceSimulation import FusedSimulationBackend
    from sampler.SimulationBasedSampler import SimulationBasedSampler
    real, seen = nh.simulate_clique, []

    def recording(ops, n, D_out, D_total, seed, device):
        seen.append((list(ops), n, D_out, D_total, seed))
        return real(ops, n, D_out, D_total, seed, device)
    monkeypatch.setattr(nh, "simulate_clique", recording)
    fs, order = eight_factor_set()
    np.random.seed(3)
    x, vs, _ = SimulationBasedSampler(fs, order).sample(1000, backend=FusedSimulationBackend(DEV))
    assert len(seen) == 1 and x.is_cuda
    ops, n, D_out, D_total, seed = seen[0]
    assert (n, D_out, D_total) == (1000, x.shape[1], x.shape[1]) and len(ops) == 8 and 0 <= seed < 2 ** 62
    angles, off = [], 0
    for v in vs:
        if v.dim == 3:
            angles.append(off + 2)
        off += v.dim
    assert off == D_out and len(angles) == 3
    cs = case("the eight-factor clique", ops, n, D_out, D_total, seed, angles=angles)
    check(cs["name"], x.cpu().numpy(), reference(cs), angles)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _bad_lists():
    """(what, records): each a runnable list with ONE field out of range.  D_total = 12: columns 0-2 A, 3-5 B, 6-7 P, 8-9 Q
    from one COPY of a [n, 10] source; outputs at 10."""
    D = 12
    base = rec(R.COPY, a=10, b=0, c=0, k=10, src=1)
    L6, L3 = [0.1, 0, 0.1, 0, 0, 0.01], [0.1, 0, 0.1]
    out = []
    for name, code, w, p in (("REL_FWD", R.REL_FWD, 3, [0] * 3 + L6), ("REL_BWD", R.REL_BWD, 3, [0] * 3 + L6),
                             ("REL_OBS", R.REL_OBS, 3, [0] * 3 + L6), ("RING", R.RING, 2, [5, 0.1]),
                             ("RANGE_OBS", R.RANGE_OBS, 2, [0.1]), ("ADA_OBS", R.ADA_OBS, 2, [0.5, 1, 1, 1, 0.1]),
                             ("NH_RING", R.NH_RING, 2, [5, 0.1, 1, 0.7]), ("NH_OBS", R.NH_OBS, 2, [0.1, 1, 0.7]),
                             ("REL_R2_FWD", R.REL_R2_FWD, 2, [1, 1] + L3), ("REL_R2_BWD", R.REL_R2_BWD, 2, [1, 1] + L3),
                             ("REL_R2_OBS", R.REL_R2_OBS, 2, [0, 0] + L3)):
        c = 0 if code in (R.REL_FWD, R.REL_BWD, R.REL_OBS) else 10      # (a 3-wide result over A: the write is in range)
        kw = dict(c=c, p=p, k=2 if code == R.ADA_OBS else 0, cand=[6, 8] if code == R.ADA_OBS else ())
        for bad in (-1, D - w + 1, 2 ** 31 - 1, -2 ** 31):
            out.append(("%s a = %d" % (name, bad), [base, rec(code, a=bad, b=3, **kw)]))
            if code in (R.REL_OBS, R.RANGE_OBS, R.NH_OBS, R.REL_R2_OBS):
                out.append(("%s b = %d" % (name, bad), [base, rec(code, a=0, b=bad, **kw)]))
            if code == R.ADA_OBS:
                for j in (0, 1):
                    kw2 = dict(kw, cand=[bad, 8] if j == 0 else [6, bad])
                    out.append(("ADA_OBS cand[%d] = %d" % (j, bad), [base, rec(code, a=0, **kw2)]))
    ada = dict(a=0, c=10, cand=[6, 8, 6, 8], p=[0.5, 1, 1, 1, 0.1])
    out += [("ADA_OBS k = %d" % k, [base, rec(R.ADA_OBS, k=k, **ada)]) for k in (0, -1, 5)]
    for what, kw in (("b = -1", dict(a=10, b=-1, k=2)), ("b + k = a + 1", dict(a=10, b=9, k=2)), ("a = 0", dict(a=0, b=0, k=1)),
                     ("k = 0", dict(a=10, b=0, k=0)), ("k = -1", dict(a=10, b=0, k=-1)), ("k = 2^31 - 1", dict(a=10, b=0, k=2 ** 31 - 1)),
                     ("c + k = D_total + 1", dict(a=10, b=0, k=3, c=10)), ("c = -1", dict(a=10, b=0, k=3, c=-1)),
                     ("a = -2^31", dict(a=-2 ** 31, b=0, k=2))):
        out.append(("COPY " + what, [base, rec(R.COPY, src=1, **dict(dict(c=10), **kw))]))
    out.append(("code 0", [base, rec(0, c=10)]))
    out.append(("code 16", [base, rec(16, c=10)]))
    return out


def test_out_of_range_ops_are_refused_before_any_launch():
    """a, b, cand[j < k], a COPY's b / k / a, k: every list with one field out of range returns NFISAM_ERR_ARG and leaves
    the output buffer (prefilled) as it was; the same lists with the field in range run."""
    import nfisam_hip as nh
    n, D = 64, 12
    src = np.random.RandomState(0).uniform(-5, 5, (n, 10)).astype(np.float32)
    buf = torch.full((n, D), SENTINEL, dtype=torch.float32, device=DEV)
    lists = _bad_lists()
    assert len(lists) > 80
    keep = upload_sources(dict(sources={1: src}))
    for what, recs in lists:
        ops, _ = device_ops(dict(ops=recs), keep=keep)
        assert launch_into(buf, ops, n, D, D, 9) == nh.ERR_ARG, what
        assert bool((buf == SENTINEL).all()), what
    # the largest values that are in range are accepted (and replayed)
    good = [rec(R.COPY, a=10, b=0, c=0, k=10, src=1), rec(R.COPY, a=10, b=8, c=10, k=2, src=1),
            rec(R.REL_OBS, a=0, b=9, c=3, p=[0] * 3 + [0.1, 0, 0.1, 0, 0, 0.01]),
            rec(R.ADA_OBS, a=10, c=11, k=2, cand=[10, 0, -5, 99], p=[0.5, 1, 1, 1, 0.1]),        # cand[j >= k] is not read
            rec(R.RING, a=10, c=10, p=[5, 0.1])]
    cs = case("largest indices in range", good, n, D, D, 9, {1: src}, angles=[2, 5])
    check(cs["name"], launch(cs), reference(cs), cs["angles"])


# ---- normalisation ---------------------------------------------------------------------------------------------------------
def wrap_pi(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


def normalize_oracle(x32, circular):
    """float64: Euclidean mean / direction of the mean resultant folded to [-pi, pi); (wrapped) deviations; their
    population std, clipped at 1e-5 -> (x_out, mean, std, resultant length per column, deviations)."""
    x = x32.astype(np.float64)
    n, D = x.shape
    mean, std, res, out, dev = np.zeros(D), np.zeros(D), np.ones(D), np.zeros((n, D)), np.zeros((n, D))
    for c in range(D):
        if circular is not None and circular[c]:
            s, co = np.sin(x[:, c]).sum(), np.cos(x[:, c]).sum()
            mu = np.arctan2(s, co)
            mu = mu - 2 * np.pi if mu >= np.pi else mu
            d = wrap_pi(x[:, c] - mu)
            res[c] = np.hypot(s, co) / n
        else:
            mu = x[:, c].mean()
            d = x[:, c] - mu
        mean[c], std[c], dev[:, c] = mu, max(d.std(), 1e-5), d
        out[:, c] = d / std[c]
    return out, mean, std, res, dev


def normalisation_input(n, D):
    """-> (x float32 [n, D], circular flags or None)."""
    rng = np.random.RandomState(100 * D + n % 97)
    side = rng.rand(n) < 0.6
    seam_p = np.where(side, 3.1, -3.1) + 0.02 * rng.randn(n)                       # clustered across the seam, mean near +pi
    seam_m = np.where(side, -3.1, 3.1) + 0.02 * rng.randn(n)                       # ... near -pi
    bimodal = np.where(rng.rand(n) < 0.65, 2.0, 2.0 - np.pi + 0.4) + 0.25 * rng.randn(n)       # resultant length ~ 0.3
    cols = [rng.randn(n), seam_p, 1e4 + 1e-2 * rng.randn(n), bimodal, np.full(n, -2.5), seam_m, -3.0 + 0.5 * rng.randn(n)]
    circ = np.array([0, 1, 0, 1, 1, 1, 1], dtype=np.uint8)
    if D == 1:
        return wrap_pi(seam_p).astype(np.float32)[:, None], np.array([1], dtype=np.uint8)
    x = np.column_stack(cols[:D])
    x[:, circ[:D] == 1] = wrap_pi(x[:, circ[:D] == 1])
    return x.astype(np.float32), circ[:D]


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("D", [1, 7])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_normalisation_equals_the_float64_oracle(n, D):
    """n around the 256-thread block and n = 1; angle columns clustered at +3.1 / -3.1 across the seam, bimodal with a
    short resultant, constant; a Euclidean column with mean 1e4 and std 1e-2; in place and out of place, equal bits."""
    import nfisam_hip as nh
    x, circ = normalisation_input(n, D)
    ref, mean, std, res, dev = normalize_oracle(x, circ)
    # the oracle alone shows that the inputs are well-posed: no vanishing resultant, no deviation at the wrap's jump
    assert res.min() >= 0.1 and np.all(np.pi - np.abs(dev[:, circ == 1]) > 1e-6)
    if D == 7 and n >= 255:
        assert 0.2 < res[3] < 0.4 and abs(std[2] - 1e-2) < 2e-3 and std[4] == 1e-5 and mean[1] > 3.1 and mean[5] < -3.1
    xd = torch.from_numpy(x).to(DEV)
    out, m, s = nh.normalize_columns(xd, circ)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)
    out, m, s = out.cpu().numpy(), m.cpu().numpy(), s.cpu().numpy()
    em, es, eo = np.abs(m - mean) / ulp32(mean), np.abs(s - std) / ulp32(std), np.maximum(np.abs(out - ref) - 1e-7, 0) / ulp32(ref)
    print("normalisation n = %d D = %d: mean %.2f ulp, std %.2f ulp, x_out %.2f ulp" % (n, D, em.max(), es.max(), eo.max()))
    assert em.max() <= 2 and es.max() <= 2 and eo.max() <= 2
    # in place
    y = torch.from_numpy(x).to(DEV)
    m2, s2 = torch.empty(D, device=DEV), torch.empty(D, device=DEV)
    cd = torch.from_numpy(circ).to(DEV)
    assert nh.lib().nfisam_normalize_columns(nh._ptr(y), n, D, nh._ptr(cd), nh._ptr(y), nh._ptr(m2), nh._ptr(s2), nh._stream()) == 0
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == out.tobytes() and m2.cpu().numpy().tobytes() == m.tobytes() and \
        s2.cpu().numpy().tobytes() == s.tobytes()


@pytest.mark.parametrize("n", [1, 257])
def test_normalisation_of_euclidean_columns_without_flags(n):
    """`circular` NULL: a column of mean 1e4 and std 1e-2 on its own (D = 1) -- the deviations are a few float32 steps of the
    input, and the sums must not lose them."""
    import nfisam_hip as nh
    x = (1e4 + 1e-2 * np.random.RandomState(n).randn(n, 1)).astype(np.float32)
    ref, mean, std, _, _ = normalize_oracle(x, None)
    out, m, s = [t.cpu().numpy() for t in nh.normalize_columns(torch.from_numpy(x).to(DEV))]
    assert np.abs(m - mean).max() <= 2 * ulp32(mean).min() and np.abs(s - std).max() <= 2 * ulp32(std).min()
    assert np.all(np.abs(out - ref) <= 2 * ulp32(ref) + 1e-7)
