"""The density direction graded per element by its forward error in float64: nsf_forward_kernel (nfisam_hip.forward, behind
separator_forward, FlowsPriorFactor.log_pdf and the hold-out validation loss) and nsf_posterior_density_kernel +
nsf_density_sum_kernel (nfisam_hip.posterior_log_density), with the grader, the cases, the points and the bound of
tests/test_density_forward_cpu.py (read its docstring first).

    max r <= 8 max(R32, 4)  over EVERY element of z, logdet, logprob, of a clique's term, its latent and log_q;
    R32: the float32 replay's largest ratio on the same inputs, R32 <= 64.

Forward: the 18 cases (D = 1 .. 20, one to eight waves, a layer stride through model_D > D).  Tolerance-free: a column with
|x| > B or NaN comes through with its own bits, a row of tail columns has log-det 0, everything else is finite (the log-density
of a row with a NaN column is NaN); a particle's bits of z, logdet and logprob depend neither on n nor on its place in the tile
(rows 0:1, 0:64, 0:65, the last row alone, the whole call twice); want_z=False leaves logdet and logprob unchanged bit for bit.
The bit-identity rows are guaranteed only from the commit on that adds this file: until then every wave added its layer's
log-det into one LDS word per particle with a float atomicAdd, in the order the waves happened to arrive (D >= 3 or L >= 2: not
a function of the inputs: two processes of that build gave sums of logprob over the same 2000 x 3 points that differ in the
ninth digit); now each wave keeps its log-det in a register and thread p adds the W partial sums in wave order.

Tree density: the six WALK_TREES at the walk's own draws plus planted rows (angles shifted by +-2 pi, columns beyond B std), in
the four-wave form; log_q carries the bits of the float32 sum of `per` in table order (`sum_in_table_order`); the same
place-independence rows.  The one-wave form (`unit_density` switches to it above 16384 blocks) on its own: the 130 draws tiled
2700 times (351 000 points, 16 455 blocks), copy 0 and the last copy graded, every copy carrying copy 0's bits -- 130 is no
multiple of 64, so the copies sit at every tile offset.

The ratios are printed per case; those of an MI355X are in profiles/density_forward_error.json (written by `write_profile`):
the largest r_z is 8.1 (L = 3, D = 7; the float32 oracle's 3.7, the largest device / replay quotient, 2.2), the largest r_ld 12.0
(D = 3 of d20h16; oracle 6.8), r_lp 2.7; a clique's term 3.8, its latent 4.1, log_q 1.3, the same in the one-wave form."""
import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_density_forward_cpu import (B, DENSITY_BLOCKS_4_WAVES, FORWARD_IDS, N, ONE_WAVE_COPIES, ONE_WAVE_TREES, PLACES, R32_MAX, WALK_TREES,
                                      _bits, bound, density_waves, exact_failures, fcase, first_rows, fixture, forward_ratio,
                                      forward_reference, sum_in_table_order, tree_ratio, tree_reference, walk_tree)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)          # a copy: the shared references are read-only


def device_forward(c, x, rows=slice(None), want_z=True):
    """-> (z, logdet, logprob) of the rows `rows`, through the whole model's parameters (model_D > D: the layer stride)."""
    kp = nh.pack(torch.from_numpy(np.ascontiguousarray(fixture()["blob_" + c.blob])).to(DEV), c.model_D, c.K, c.H, c.L)
    z, ld, lp = nh.forward(dev(x[rows]), kp, c.K, c.H, B, c.L, want_z=want_z, want_logdet=True, want_logprob=True, model_D=c.model_D)
    return (z.cpu().numpy() if want_z else None), ld.cpu().numpy(), lp.cpu().numpy()


def measure_forward(name):
    c, ref = fcase(name), forward_reference(name)
    z, ld, lp = device_forward(c, ref["x"])
    r_z, r_ld, r_lp = forward_ratio(ref["ref"], z, ld, lp)
    m = dict(case=name, D=c.D, K=c.K, H=c.H, L=c.L, model_D=c.model_D, waves=min(c.D, 8))
    for k, r in (("z", r_z), ("ld", r_ld), ("lp", r_lp)):
        m["R32_" + k], m["device_r_" + k] = ref["R32_" + k], float(r.max())
    return m, z, ld, lp


@pytest.mark.parametrize("name", FORWARD_IDS)
def test_forward_z_log_det_and_log_density_by_forward_error(name):
    c, ref = fcase(name), forward_reference(name)
    m, z, ld, lp = measure_forward(name)
    print("%-16s r_z: device %6.2f  oracle %5.2f   r_ld: device %6.2f  oracle %5.2f   r_lp: device %6.2f  oracle %5.2f"
          % (name, m["device_r_z"], m["R32_z"], m["device_r_ld"], m["R32_ld"], m["device_r_lp"], m["R32_lp"]))
    assert max(m["R32_z"], m["R32_ld"], m["R32_lp"]) <= R32_MAX                  # the condition on the inputs
    assert not exact_failures(ref["x"], z, ld, lp, c.L), exact_failures(ref["x"], z, ld, lp, c.L)
    if c.D == 1:                                                                  # L = 1: a tail dim adds exactly 0
        assert c.L == 1 and np.all(ld[~(np.abs(ref["x"][:, 0]) <= np.float32(B))] == 0.0)
    for k in ("z", "ld", "lp"):
        assert m["device_r_" + k] <= bound(m["R32_" + k]), (k, m)
    # a particle's bits depend neither on n nor on its place in the tile, nor on the call (PLACES ends with the whole call again)
    for rows in PLACES:
        zs, lds, lps = device_forward(c, ref["x"], rows)
        assert np.array_equal(_bits(zs), _bits(z[rows])), (name, rows)
        assert np.array_equal(_bits(lds), _bits(ld[rows])) and np.array_equal(_bits(lps), _bits(lp[rows])), (name, rows)
    _, ld0, lp0 = device_forward(c, ref["x"], want_z=False)
    assert np.array_equal(_bits(ld0), _bits(ld)) and np.array_equal(_bits(lp0), _bits(lp))


# ------------------------------------------------------------------ the tree density -----
def _table(name):
    """The clique table of the tree as `posterior_log_density` takes it -> (table, cols, obs, max_D, tensors kept alive)."""
    K, H, L, total, cliques = walk_tree(name)
    rows, cols, obs, keep = [], [], [], []
    for q in cliques:
        t = (nh.pack(torch.from_numpy(np.ascontiguousarray(q.blob)).to(DEV), q.D_model, K, H, L), dev(q.mean), dev(q.std),
             torch.from_numpy(q.circ.astype(np.uint8)).to(DEV))
        keep.append(t)
        r = np.zeros(1, dtype=nh.POST_DTYPE)
        r["kparams"], r["mean"], r["std"], r["circular"] = (a.data_ptr() for a in t)
        r["D_model"], r["n_obs"], r["n_sep"], r["n_frontal"] = q.D_model, len(q.obs), len(q.sep), len(q.front)
        r["obs_off"], r["sep_off"], r["front_off"] = len(obs), len(cols), len(cols) + len(q.sep)
        obs.extend(float(v) for v in q.obs)
        cols.extend(q.sep + q.front)
        rows.append(r)
    return np.concatenate(rows), np.array(cols, dtype=np.int32), np.array(obs, dtype=np.float32), max(q.D_model for q in cliques), keep


def device_density(name, X, tab=None):
    """-> (log_q [n], per [n_cliques, n], latent [total, n]) at the points X [n, total] (a device tensor or float32 numpy)."""
    K, H, L, total, cliques = walk_tree(name)
    table, cols, obs, max_D, keep = tab or _table(name)
    S = X if torch.is_tensor(X) else dev(X)
    lq, per, lat = nh.posterior_log_density(table, cols, obs, S, max_D, K, H, B, L, DEV, per_clique=True, latent=True)
    return lq.cpu().numpy(), per.cpu().numpy(), lat.cpu().numpy()


def measure_density(name, tab=None):
    ref = tree_reference(name)
    lq, per, lat = device_density(name, ref["X"], tab)
    r_per, r_lat, r_q = tree_ratio(ref["refs"], per, lat, lq)
    waves, blocks = density_waves(ref["X"].shape[0], per.shape[0])
    return dict(tree=name, waves=waves, blocks=blocks, n=ref["X"].shape[0], R32_per=ref["R32_per"], R32_lat=ref["R32_lat"],
                R32_q=ref["R32_q"], device_r_per=r_per, device_r_lat=r_lat, device_r_q=r_q), lq, per, lat


def _check_density(m):
    assert max(m["R32_per"] + m["R32_lat"] + [m["R32_q"]]) <= R32_MAX            # the condition on the inputs
    for k in ("per", "lat"):
        for r, r32 in zip(m["device_r_" + k], m["R32_" + k]):
            assert r <= bound(r32), (k, m)
    assert m["device_r_q"] <= bound(m["R32_q"]), m


def _show(m):
    print("%-14s W = %d, %5d blocks  term: device %s  replay %s   latent: device %s  replay %s   log_q: device %.2f  replay %.2f"
          % (m["tree"], m["waves"], m["blocks"], " ".join("%5.2f" % r for r in m["device_r_per"]), " ".join("%4.2f" % r for r in m["R32_per"]),
             " ".join("%5.2f" % r for r in m["device_r_lat"]), " ".join("%4.2f" % r for r in m["R32_lat"]), m["device_r_q"], m["R32_q"]))


@pytest.mark.parametrize("name", WALK_TREES)
def test_tree_density_terms_latents_and_log_q_by_forward_error(name):
    ref, tab = tree_reference(name), _table(name)
    m, lq, per, lat = measure_density(name, tab)
    _show(m)
    assert m["waves"] == 4
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(lat)) and np.all(np.isfinite(lq))
    _check_density(m)
    assert np.array_equal(_bits(lq), _bits(sum_in_table_order(per)))
    total_front = sum(len(q.front) for q in walk_tree(name)[4])
    n = ref["X"].shape[0]
    for rows in (slice(0, 1), slice(0, 64), slice(0, 65), slice(n - 1, n), slice(0, n)):
        lqs, pers, lats = device_density(name, ref["X"][rows], tab)
        assert np.array_equal(_bits(lqs), _bits(lq[rows])) and np.array_equal(_bits(pers), _bits(per[:, rows])), (name, rows)
        assert np.array_equal(_bits(lats[:total_front]), _bits(lat[:total_front, rows])), (name, rows)


def measure_one_wave(name, tab=None):
    """The walk's 130 draws tiled ONE_WAVE_COPIES times on the device -> (ratios of copy 0 and of the last copy, the outputs as
    [.., copies, 130])."""
    ref = tree_reference(name)
    nc = len(ref["refs"])
    n = N * ONE_WAVE_COPIES
    X = dev(ref["X"][:N]).repeat(ONE_WAVE_COPIES, 1)
    lq, per, lat = device_density(name, X, tab)
    waves, blocks = density_waves(n, nc)
    lq, per, lat = lq.reshape(ONE_WAVE_COPIES, N), per.reshape(nc, ONE_WAVE_COPIES, N), lat.reshape(-1, ONE_WAVE_COPIES, N)
    refs = first_rows(ref["refs"], N)
    out = []
    for copy in (0, ONE_WAVE_COPIES - 1):
        r_per, r_lat, r_q = tree_ratio(refs, per[:, copy], lat[:, copy], lq[copy])
        out.append(dict(tree=name, waves=waves, blocks=blocks, n=n, copy=copy, R32_per=ref["R32_per"], R32_lat=ref["R32_lat"],
                        R32_q=ref["R32_q"], device_r_per=r_per, device_r_lat=r_lat, device_r_q=r_q))
    return out, lq, per, lat


@pytest.mark.parametrize("name", ONE_WAVE_TREES)
def test_the_one_wave_form_of_the_tree_density_on_its_own(name):
    """R32 is the replay's over the whole point set of `tree_reference`, the walk's draws among it."""
    nc = len(walk_tree(name)[4])
    assert density_waves(N * ONE_WAVE_COPIES, nc)[1] > DENSITY_BLOCKS_4_WAVES and density_waves(N * ONE_WAVE_COPIES, nc)[0] == 1
    assert density_waves(N, nc) == (4, 3 * nc)
    ms, lq, per, lat = measure_one_wave(name)
    for m in ms:
        _show(m)
        _check_density(m)
    assert np.array_equal(_bits(lq), np.broadcast_to(_bits(lq[:1]), lq.shape))
    assert np.array_equal(_bits(per), np.broadcast_to(_bits(per[:, :1]), per.shape))
    assert np.array_equal(_bits(lat), np.broadcast_to(_bits(lat[:, :1]), lat.shape))
    assert np.array_equal(_bits(lq[0]), _bits(sum_in_table_order(per[:, 0])))


def write_profile(path):
    """Every case's ratios -> the JSON of profiles/density_forward_error.json.  From the repository root, on an MI355X:
        PYTHONPATH=nf-isam_amd:.:tests python tests/test_density_forward_gpu.py profiles/density_forward_error.json"""
    import json
    fwd = [measure_forward(name)[0] for name in FORWARD_IDS]
    tree = [measure_density(name)[0] for name in WALK_TREES]
    one = [m for name in ONE_WAVE_TREES for m in measure_one_wave(name)[0]]
    quot = [(m["device_r_" + k] / m["R32_" + k], m["case"], "r_" + k) for m in fwd for k in ("z", "ld", "lp")]
    for m in tree + one:
        what = "%s / W = %d" % (m["tree"], m["waves"])
        quot += [(a / b, "%s / clique %d" % (what, j), "r_" + k) for k in ("per", "lat")
                 for j, (a, b) in enumerate(zip(m["device_r_" + k], m["R32_" + k]))]
        quot.append((m["device_r_q"] / m["R32_q"], what, "r_q"))
    q = max(quot)

    def rnd(o):
        if isinstance(o, float):
            return round(o, 3)
        if isinstance(o, list):
            return [rnd(v) for v in o]
        return {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else o
    out = {
        "what": "forward error of every output of nfisam_nsf_forward and nfisam_nsf_posterior_log_density and of the float32 replays (host), in "
                "float64: tests/test_density_forward_cpu.py (grader, cases), tests/test_density_forward_gpu.py (this writer)",
        "ratio": "r_z = |z - fwd64| / (2^-24 L s_z), s_z = (B + |fwd64|) + slope (B + |x|); r_ld = |ld - sum lad64| / (2^-24 L s_ld), s_ld = "
                 "sum (1 + |d lad/dx| (B + |x|)); r_lp = |lp - lp64| / (2^-24 L (s_ld + sum (|fwd64| s_z + fwd64^2 / 2 + 0.92))); r_per: r_lp over "
                 "a clique's frontal dims, + sum |log std| in the scale, the normalisation's (|x_raw| + |mean| + pi circular) / std joining "
                 "B + |x|; r_lat: r_z of the latent; r_q: log_q against the sum of the cliques' terms; the largest over all elements of a case "
                 "(B = %g)" % B,
        "bound": "device <= 8 max(R32, 4), R32 <= %g (R32: the float32 replay's ratio on the same inputs)" % R32_MAX,
        "device": torch.cuda.get_device_name(0),
        "largest_device_over_replay": {"quotient": q[0], "case": q[1], "ratio": q[2]},
        "largest_device_ratio": {"forward_r_z": max(m["device_r_z"] for m in fwd), "forward_r_ld": max(m["device_r_ld"] for m in fwd),
                                 "forward_r_lp": max(m["device_r_lp"] for m in fwd),
                                 "tree_r_per": max(max(m["device_r_per"]) for m in tree + one),
                                 "tree_r_lat": max(max(m["device_r_lat"]) for m in tree + one),
                                 "tree_r_q": max(m["device_r_q"] for m in tree + one)},
        "forward": fwd, "tree_four_waves": tree, "tree_one_wave": one}
    with open(path, "w") as f:
        json.dump(rnd(out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    import sys
    write_profile(sys.argv[1])
