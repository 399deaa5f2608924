"""Marginal posterior densities on a final tree: a dataset end to end (run_plaza1.py's defaults, as scripts/sample_modes.py), then
at n = 500 and 2000 posterior points:
  * device us of NFiSAM.posterior_marginal_density(samples, curves=500) -- every coordinate of every variable on a 500-point
    grid -- and of (samples, maps=(64, 64)), from HIP events around the whole call (the call computes the covariances, forms the
    bandwidths and grids on the host, uploads its tables and copies the densities back, so host work between launches is inside
    the window), and their wall us,
  * wall us of posterior_marginal_density(n=n, curves=500) (its own device draw) beside the walk alone: the walk's share,
  * device us of the C entry alone on the curves' table (matrix and grid in place, tables uploaded per call, outputs allocated),
    and its float64 kernel evaluations per us (two sweeps: each pair's exponent is formed twice, its exp once),
  * the truth scores of the call (mean NLPD, coverage) against the dataset's ground truth, for the record,
  * for scale, on the host: scipy.stats.gaussian_kde(column).pdf(grid) per coordinate, what the reference's kde_plot_grid does,
    on the first 60 coordinates and scaled up, and the largest relative deviation of the device's curves from scipy's there
    (where scipy is missing, that is recorded instead),
  * with --tests: the largest error / bound ratios over the GPU tests' cases and the measured ulp errors of the device's exp
    and log (the EXP_ULP and LOG_ULP the tests' bound is built from),
  * the compiler's resource figures of the unit (recorded below from its report).
No time is asserted or aimed at: there is nothing to compare with but the host path recorded next to it.
Prints one JSON object and merges it under the dataset's name into out.json.
usage: sample_density.py [--tests] [--updates=K (default: all)] [dataset (default Plaza1EFG)] [out.json (default profiles/density.json)]"""
import contextlib, io, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from utils import Statistics as ST

REPS, WARM = 20, 5
G_CURVE, G_MAP = 500, (64, 64)
# hipcc -O3 -ffp-contract=fast --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on sample_density.hip
RESOURCES = dict(density_kernel=dict(vgprs=122, agprs=0, sgprs=106, sgpr_spills_to_vgpr_lanes=8, scratch_bytes_per_lane=0,
                                     lds_bytes=9448, waves_per_simd=4))
flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
dataset = args[0] if args else "Plaza1EFG"
out_path = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "density.json")
np.random.seed(0); torch.manual_seed(0)
nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", dataset, "factor_graph.fg"), "fg")
steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=5)
all_updates = len(steps)
for a in flags:
    if a.startswith("--updates="):
        steps = steps[:int(a.split("=")[1])]
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
print("%s end to end: %.1f s" % (dataset, run_s), flush=True)


def stats(ts):
    ts = np.asarray(ts[-REPS:])
    return dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))


def timed(f):
    """(device us between events around f, wall us of f with a final synchronise): WARM + REPS calls."""
    dev, wall = [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(WARM + REPS):
        torch.cuda.synchronize()
        a = time.perf_counter()
        ev0.record()
        f()
        ev1.record()
        ev1.synchronize()
        wall.append((time.perf_counter() - a) * 1e6)
        dev.append(ev0.elapsed_time(ev1) * 1e3)
    return stats(dev), stats(wall)


order = list(solver.elimination_ordering)
pcol, total_dim = solver._post_columns()
known = {v: np.asarray(truth[v], dtype=np.float64) for v in order if v in truth} if isinstance(truth, dict) else {}
out = dict(dataset=dataset, updates=len(steps), updates_of_the_dataset=all_updates, end_to_end_s=run_s, variables=len(order),
           total_dim=total_dim, stat="median / min / max of the replays after the warm-ups that every n records, us",
           arguments=dict(curves=G_CURVE, maps=list(G_MAP), bandwidth="scott"))
try:
    from scipy.stats import gaussian_kde
except ImportError:
    gaussian_kde = None
    out["host_scipy"] = "scipy is not installed here: no host time recorded"

for n in (500, 2000):
    REPS, WARM = (20, 5) if n == 500 else (5, 2)
    S = solver.posterior_launch(n)["S"]                              # [n, total_dim] on the device
    smp = {v: S[:, pcol[v]:pcol[v] + v.dim] for v in order}          # device views: what posterior_marginal_density(samples) takes
    r = dict(matrix_bytes=int(S.numel() * 4), reps=REPS, warmups=WARM, curve_blocks=total_dim, map_blocks=sum(v.dim >= 2 for v in order))
    r["curves_device_us"], r["curves_wall_us"] = timed(lambda: solver.posterior_marginal_density(samples=smp, curves=G_CURVE))
    r["maps_device_us"], r["maps_wall_us"] = timed(lambda: solver.posterior_marginal_density(samples=smp, maps=G_MAP))
    r["own_draw_device_us"], r["own_draw_wall_us"] = timed(lambda: solver.posterior_marginal_density(n=n, curves=G_CURVE))
    r["walk_alone_device_us"], r["walk_alone_wall_us"] = timed(lambda: solver.posterior_launch(n))
    r["walk_share_of_own_draw_wall"] = r["walk_alone_wall_us"]["median"] / r["own_draw_wall_us"]["median"]
    got = solver.posterior_marginal_density(samples=smp, curves=G_CURVE)

    # the entry alone on the curves' table: one 1-column block per coordinate, its own 500 queries
    St = S.t().contiguous()
    grid = np.stack([got["curves"][v][c]["x"] for v in order for c in range(v.dim)]).astype(np.float32)
    hs = np.array([got["curves"][v][c]["h"] for v in order for c in range(v.dim)])
    cols = np.concatenate([np.arange(pcol[v], pcol[v] + v.dim) for v in order]).astype(np.int32)
    wrap = np.concatenate([[int(bool(f)) for f in v.circular_dim_list] for v in order]).astype(np.uint8)
    table = nh.pack_density_blocks(np.ones(cols.size), [np.array([[1.0 / h]]) for h in hs])
    Qt = torch.from_numpy(grid).to(St.device)
    qrows = np.arange(cols.size, dtype=np.int32)
    nh.check_density_blocks(table, qrows, cols, cols.size, total_dim, wrap)
    r["entry_device_us"], _ = timed(lambda: nh.sample_density_t(Qt, St, table, qrows, cols, wrap, want_density=True, checked=True))
    pairs = float(cols.size) * G_CURVE * n
    r["pairs"] = pairs
    r["pairs_per_us"] = pairs / r["entry_device_us"]["median"]
    if known:
        graded = solver.posterior_marginal_density(samples=smp, truth=known)
        r["truth"] = dict(graded=len(graded["nlpd"]), mean_nlpd=graded["mean_nlpd"], coverage={str(k): v for k, v in graded["coverage"].items()})
    if gaussian_kde is not None:
        H = S.cpu().numpy().astype(np.float64)
        some, worst, refs = 60, 0.0, {}
        t1 = time.perf_counter()
        for e in range(some):
            if not wrap[e]:                                          # (scipy has no circular kernel)
                refs[e] = gaussian_kde(H[:, cols[e]]).pdf(grid[e].astype(np.float64))
        host_us = (time.perf_counter() - t1) * 1e6
        flat = [got["curves"][v][c]["density"] for v in order for c in range(v.dim)]
        for e, ref in refs.items():
            worst = max(worst, float(np.max(np.abs(flat[e] - ref) / np.maximum(ref, 1e-300) * (ref > 1e-12))))
        used = int(np.sum(wrap[:some] == 0))
        r["host_scipy_wall_us_scaled_from_%d_coordinates" % used] = host_us * cols.size / max(used, 1)
        r["largest_relative_deviation_from_scipy_where_density_above_1e-12"] = worst
    print("n = %d: curves %.0f us device, %.0f us wall; maps %.0f us device; entry %.0f us" % (
        n, r["curves_device_us"]["median"], r["curves_wall_us"]["median"], r["maps_device_us"]["median"], r["entry_device_us"]["median"]),
        flush=True)
    out["n%d" % n] = r

if "--tests" in flags:                                              # error / bound over the GPU tests' own cases
    import test_sample_density_gpu as G
    recorded = (G.EXP_ULP, G.LOG_ULP)
    G.EXP_ULP = G.LOG_ULP = float("inf")                            # (measured here, not asserted)
    with contextlib.redirect_stdout(io.StringIO()):                 # (the tests print every figure)
        G.test_device_exp_and_log_ulps()
    ulps = dict(device_exp_largest_error_ulp=G._worst.pop("device_exp_ulp"), device_log_largest_error_ulp=G._worst.pop("device_log_ulp"))
    G.EXP_ULP, G.LOG_ULP = recorded
    G._worst.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        for d in (1, 2, 3, 6):
            for n in (1, 31, 32, 33, 127, 128, 129, 130, 300):
                G.test_values_at_every_shape(n, d)
        G.test_a_table_of_forty_blocks()
        for k in (0, 1, 2):
            for rule in ("scott", "silverman"):
                G.test_fixture_cases_against_scipy(k, rule)
        G.test_the_heading_seam()
        for n in (2, 65, 130, 200):
            G.test_exclude_self(n)
        G.test_a_zero_weight_is_a_deleted_point()
        G.test_nan_queries_and_far_queries()
        G.test_statistics_sample_density_and_hpd_level()
        G.test_leave_one_out_selection_on_the_bimodal_set()
    out["largest_ratio"] = dict(error_over_bound_in_the_gpu_tests=dict(G._worst), exp_ulp_the_tests_take=G.EXP_ULP,
                                log_ulp_the_tests_take=G.LOG_ULP, rule="the bounds of tests/test_sample_density_gpu.py (its docstring states them)",
                                **ulps)
out["resources"] = RESOURCES
print(json.dumps(out))
doc = {}
if os.path.exists(out_path):
    with open(out_path) as f:
        doc = json.load(f)
doc[dataset] = out
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
