"""Two-sample MMD on the final Plaza1 tree: Plaza1 end to end (run_plaza1.py's defaults, as scripts/factor_density.py), then
the joint xy block plus every variable's xy marginal -- the posterior against a second draw of itself, the stand-in for a
reference solution of the same layout -- at n = m = 500 and 2000:
  * device us of nfisam_sample_mmd from HIP events around the call (tables uploaded, matrices in place; median of 20 calls
    after one warm-up call),
  * wall us of NFiSAM.posterior_mmd(reference, samples) and of NFiSAM.posterior_mmd(reference) (its own device draw),
  * the baseline: the numpy `utils.Statistics.mmd` loop over the same blocks on the same machine (one pass: it takes minutes
    at 2000), with the points already on the host,
  * the largest relative deviation of the device sums from the float64 oracle (direct differences at the float32 points;
    every block at 500, the joint block and the first 40 marginals at 2000), and of the device `mmd` values from the loop's.
Prints one JSON object.   usage: sample_mmd.py [out.json]"""
import ctypes as C
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT)
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from utils import Statistics as ST

REPS = 20
DEV = "cuda:0"
np.random.seed(0); torch.manual_seed(0)
nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", "Plaza1EFG", "factor_graph.fg"), "fg")
steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=5)
solver = NFiSAM(NFiSAMArgs(num_knots=9, flow_iterations=2000, local_sample_num=2000, learning_rate=.01, hidden_dim=8,
                           cuda_training=True, elimination_method="pose_first", training_set_frac=1.0, loss_delta_tol=.01,
                           average_window=50))
t0 = time.time()
for vs, fs in steps:
    for v in vs: solver.add_node(v)
    for f in fs: solver.add_factor(f)
    solver.update_physical_and_working_graphs()
    solver.incremental_inference()
torch.cuda.synchronize()
run_s = time.time() - t0
print("Plaza1 end to end: %.1f s" % run_s, flush=True)


def median_after_first(f, reps=REPS):
    ts = [f() for _ in range(reps + 1)]
    return float(np.median(ts[1:]))


def oracle_sums(x, y, inv, rows=16):
    """{Sxx, Syy, Sxy} in float64 by direct differences, `rows` rows of the first set at a time."""
    out = []
    for a, b in ((x, x), (y, y), (x, y)):
        s = 0.0
        for r in range(0, a.shape[0], rows):
            diff = a[r:r + rows, None, :] - b[None, :, :]
            s += np.exp(-inv * np.einsum("ijk,ijk->ij", diff, diff)).sum()
        out.append(s)
    return np.array(out)


order = list(solver.elimination_ordering)
out = dict(dataset="Plaza1EFG", updates=len(steps), end_to_end_s=run_s, variables=len(order), blocks=len(order) + 1,
           joint_columns=2 * len(order), estimator="mmd (k_sigma2 = 1), xy columns", reps=REPS,
           stat="median of %d calls after one warm-up call; the numpy loop once" % REPS)
pcol, total_dim = solver._post_columns()
for n in (500, 2000):
    solver._args.posterior_sample_num = n
    smp = {v: np.array(a) for v, a in solver.sample_posterior().items()}
    ref = {v: np.array(a) for v, a in solver.sample_posterior().items()}
    got = solver.posterior_mmd(ref, smp)
    r = dict(joint=got["joint"], marginal_mean=got["marginal_mean"], floor=got["floor"],
             marginals_nan=int(np.sum(np.isnan(list(got["marginal"].values())))))

    def wall_given():
        a = time.perf_counter()
        solver.posterior_mmd(ref, smp)
        return (time.perf_counter() - a) * 1e6

    def wall_drawn():
        a = time.perf_counter()
        solver.posterior_mmd(ref, n=n)
        return (time.perf_counter() - a) * 1e6
    r["posterior_mmd_wall_us"] = median_after_first(wall_given)
    r["posterior_mmd_own_draw_wall_us"] = median_after_first(wall_drawn)
    # the same launch by hand: xy columns, the reference in the solver's column layout
    X = np.zeros((n, total_dim), dtype=np.float32)
    Y = np.zeros((n, total_dim), dtype=np.float32)
    for v in order:
        X[:, pcol[v]:pcol[v] + v.dim] = smp[v]
        Y[:, pcol[v]:pcol[v] + v.dim] = ref[v]
    xy = [[pcol[v], pcol[v] + 1] for v in order]
    blocks = [[c for b in xy for c in b]] + xy
    cols = np.concatenate([np.asarray(b, dtype=np.int32) for b in blocks])
    table = nh.pack_mmd_blocks([len(b) for b in blocks], np.ones(len(blocks)))
    nh.check_mmd_blocks(table, cols, cols, total_dim, total_dim)
    Xt, Yt = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV), torch.from_numpy(np.ascontiguousarray(Y.T)).to(DEV)
    table_d, cols_d = nh.upload(table.view(np.uint8).reshape(-1), cols, device=DEV, cached=True)
    count = int(nh.lib().nfisam_sample_mmd_scratch_count(n, n, len(blocks)))
    scratch = torch.empty(count, dtype=torch.float64, device=DEV)
    sums = torch.empty(len(blocks), 3, dtype=torch.float64, device=DEV)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def kernel():
        ev0.record()
        nh._check(nh.lib().nfisam_sample_mmd(nh._ptr(Xt), total_dim, n, nh._ptr(Yt), total_dim, n,
                                             table.ctypes.data_as(C.c_void_p), C.c_void_p(table_d.data_ptr()), len(blocks),
                                             nh._ptr(cols_d), nh._ptr(cols_d), int(cols.size), None, None, nh._ptr(sums),
                                             nh._ptr(scratch), nh._stream()), "nfisam_sample_mmd")
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3
    r["kernel_us"] = median_after_first(kernel)
    r["scratch_doubles"] = count
    dev_sums = sums.cpu().numpy()
    dev_vals = ST.mmd_from_sums(dev_sums, n, n, "mmd")
    r["kernel_equals_solver_call"] = bool(np.array_equal(dev_vals, np.array([got["joint"]] + [got["marginal"][v] for v in order]),
                                                         equal_nan=True))
    print("n = %d: kernel %.0f us, posterior_mmd %.0f us" % (n, r["kernel_us"], r["posterior_mmd_wall_us"]), flush=True)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    a = time.perf_counter()
    host = []
    for k, b in enumerate(blocks):
        host.append(ST.mmd(X64[:, b], Y64[:, b])[0])
        if k % 200 == 0:
            print("  numpy loop: block %d of %d" % (k, len(blocks)), flush=True)
    r["numpy_loop_wall_us"] = (time.perf_counter() - a) * 1e6
    host = np.array(host)
    both = np.isfinite(host) & np.isfinite(dev_vals)
    r["nan_pattern_equal"] = bool(np.array_equal(np.isnan(host), np.isnan(dev_vals)))
    r["max_rel_diff_of_mmd_vs_numpy_loop"] = float(np.max(np.abs(dev_vals[both] - host[both]) / host[both]))
    r["speedup_vs_numpy_kernel"] = r["numpy_loop_wall_us"] / r["kernel_us"]
    r["speedup_vs_numpy_wall"] = r["numpy_loop_wall_us"] / r["posterior_mmd_wall_us"]
    checked = range(len(blocks)) if n == 500 else range(41)
    worst = 0.0
    for k in checked:
        o = oracle_sums(X64[:, blocks[k]], Y64[:, blocks[k]], 0.5)
        worst = max(worst, float(np.max(np.abs(dev_sums[k] - o) / o)))
        if k % 200 == 0:
            print("  oracle: block %d" % k, flush=True)
    r["max_rel_dev_of_sums_vs_float64_oracle"] = worst
    r["oracle_blocks_checked"] = len(checked)
    out["n%d" % n] = r

# the deviation on the GPU test's table (14 blocks, every (m, n) of the test)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_sample_mmd_gpu as G
x, y = G._data()
tb = G._table()
worst = 0.0
for m in (1, 63, 64, 65, 130):
    for n in (1, 64, 200):
        dev = nh.mmd_sums(x[:m], y[:n], *G._arrays(tb), device=DEV).cpu().numpy()
        o = G._oracle(x[:m], y[:n], tb)
        worst = max(worst, float(np.max(np.abs(dev - o) / np.maximum(o, 1e-300))))
out["max_rel_dev"] = dict(test_table=worst, plaza1_n500=out["n500"]["max_rel_dev_of_sums_vs_float64_oracle"],
                          plaza1_n2000=out["n2000"]["max_rel_dev_of_sums_vs_float64_oracle"])
out["test_bound"] = dict(rtol=G.RTOL, atol=G.ATOL, rule="the error analysis of the issue, not the measurement")
print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
