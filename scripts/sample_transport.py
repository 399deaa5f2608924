"""The sliced Wasserstein distance: what NFiSAM.posterior_transport says on the small range problem, and what the device
call costs next to the host route.
  * small range problem, its first two updates at 200 flow iterations (the setting of the tests): a stored draw against a
    second draw of the posterior, and against itself with landmark L1 moved by (0.5, 0) -- printed, wall ms of a call;
  * timing, at the shape of a Plaza1-size graph (778 variables: a 1556-column joint block plus 778 two-column blocks, 64
    directions, p = 2) with synthetic points near 100 +- 1.5, the second set shifted by 0.4, at n = m = 500 and 2000:
      new:   device us of nfisam_hip.sliced_transport_t from HIP events around the call (matrices in place; the upload of
             the tables and directions is inside);
      numpy: wall us of the host route -- both matrices copied out, then per block one projection X[:, cols] @ D.T and one
             `np.sort` per set over all its directions, the mean |a_(i) - b_(i)|^2;
    the two alternate, ROUNDS rounds after one warm-up round; medians, their ratio, and the largest relative difference
    between the two routes' slices.
Prints one JSON object; with a path, stores it there as `small_range` and `timing` (other keys of the file are kept).
usage: sample_transport.py [out.json]"""
import json, os, random, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT)
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from utils import Statistics as ST

ROUNDS, DIRS, P, VARS = 5, 64, 2, 778
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
out = dict(device=torch.cuda.get_device_name(0))

# ---- the small range problem ----------------------------------------------------------------------------------------------------
fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
kwargs = json.loads(str(fx["arguments"]))
kwargs["cuda_training"] = True
kwargs["flow_iterations"] = 200
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "factor_graph.fg")
    with open(path, "w") as f:
        f.write(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    nodes, truth, factors = graph_file_parser(path, "fg", prior_cov_scale=0.1)
steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))[:2]
solver = NFiSAM(NFiSAMArgs(**kwargs))
for vs, fs in steps:
    for v in vs: solver.add_node(v)
    for f in fs: solver.add_factor(f)
    solver.update_physical_and_working_graphs()
    solver.incremental_inference()
order = list(solver.elimination_ordering)
first = {v: np.array(a) for v, a in solver.sample_posterior().items()}
second = {v: np.array(a) for v, a in solver.sample_posterior().items()}
lm = next(v for v in order if v.name == "L1")
moved = dict(first)
moved[lm] = first[lm] + np.array([0.5, 0.0])


def named(res):
    r = {k: res[k] for k in ("joint", "marginal_mean", "marginal_max", "m", "n", "p", "directions")}
    r["marginal"] = {v.name: a for v, a in res["marginal"].items()}
    r["max_sliced"] = {(v if isinstance(v, str) else v.name): a for v, a in res["max_sliced"].items()}
    r["axes"] = {v.name: [float(x) for x in a] for v, a in res["axes"].items()}
    return r


small = {}
for name, ref in (("second_draw", second), ("L1_moved_by_half_a_metre", moved)):
    solver.posterior_transport(ref, first)                             # (one warm-up call)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = solver.posterior_transport(ref, first)
    small[name] = dict(named(res), wall_ms=(time.perf_counter() - t0) * 1e3)
    print("small range, %s:" % name, small[name], flush=True)
# the host's word on the largest figure above: L1's exact per-axis W_2 and W_1 between the two draws by numpy, and what the draws hold
a, b = np.sort(first[lm][:, :2].astype(np.float64), axis=0), np.sort(second[lm][:, :2].astype(np.float64), axis=0)
small["L1_between_the_two_draws_by_numpy"] = dict(
    w2_axes=[float(x) for x in np.sqrt(((a - b) ** 2).mean(0))], w1_axes=[float(x) for x in np.abs(a - b).mean(0)],
    w1_axes_device=[float(x) for x in solver.posterior_transport(second, first, variables=[lm], p=1, joint=False)["axes"][lm]],
    std=[float(x) for x in first[lm][:, :2].std(0)], largest_abs=[float(x) for x in np.abs(first[lm][:, :2]).max(0)],
    median_abs_deviation=[float(x) for x in np.median(np.abs(first[lm][:, :2] - np.median(first[lm][:, :2], 0)), 0)])
print("small range, L1 by numpy:", small["L1_between_the_two_draws_by_numpy"], flush=True)
out["small_range"] = dict(updates=len(steps), flow_iterations=200, **small)


# ---- the device call against the host route -------------------------------------------------------------------------------------
def device_us(f):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    r = f()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) * 1e3, r


width = 2 * VARS
xy = [np.array([2 * k, 2 * k + 1]) for k in range(VARS)]
cols = [np.arange(width)] + xy
tab = ST.transport_tables([(c, c, np.zeros(c.size, dtype=np.uint8)) for c in cols], DIRS, 0, False)
nh.check_transport_blocks(tab["blocks"], tab["xcols"], tab["ycols"], width, width, tab["dirs"])
dirs = [ST.transport_directions(c.size, DIRS, 0) for c in cols]
timing = dict(blocks=len(cols), joint_columns=width, directions=DIRS, p=P, slices=int(tab["blocks"]["n_dirs"].sum()), rounds=ROUNDS,
              stat="new and numpy alternate; median of %d rounds after one warm-up round" % ROUNDS)
for n in (500, 2000):
    rng = np.random.RandomState(n)
    Xt = torch.from_numpy((rng.standard_normal((width, n)) * 1.5 + 100.0).astype(np.float32)).to(DEV)
    Yt = torch.from_numpy((rng.standard_normal((width, n)) * 1.5 + 100.4).astype(np.float32)).to(DEV)

    def new():
        return nh.sliced_transport_t(Xt, Yt, tab["blocks"], tab["xcols"], tab["ycols"], tab["dirs"], P, checked=True)

    def host():
        X, Y = Xt.cpu().numpy().T.astype(np.float64), Yt.cpu().numpy().T.astype(np.float64)
        res = []
        for c, D in zip(cols, dirs):
            a, b = np.sort(X[:, c] @ D.T, axis=0), np.sort(Y[:, c] @ D.T, axis=0)
            res.append(((a - b) ** 2).mean(0))
        return np.concatenate(res)

    new_us, host_us = [], []
    for k in range(ROUNDS + 1):
        t_new, got = device_us(new)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host()
        t_host = (time.perf_counter() - t0) * 1e6
        if k:
            new_us.append(t_new), host_us.append(t_host)
    r = dict(new_us=float(np.median(new_us)), numpy_us=float(np.median(host_us)), new_us_rounds=new_us, numpy_us_rounds=host_us)
    r["numpy_over_new"] = r["numpy_us"] / r["new_us"]
    r["new_ns_per_slice_point"] = r["new_us"] * 1e3 / (timing["slices"] * 2.0 * n)
    r["max_relative_difference"] = float(np.max(np.abs(got.cpu().numpy() - want) / want))
    print("n = m = %d: new %.0f us, numpy %.0f us, ratio %.1f, largest relative difference %.2g"
          % (n, r["new_us"], r["numpy_us"], r["numpy_over_new"], r["max_relative_difference"]), flush=True)
    timing["n%d" % n] = r
out["timing"] = timing

print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    doc = json.load(open(args[0])) if os.path.exists(args[0]) else {}
    doc.update(out)
    with open(args[0], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
