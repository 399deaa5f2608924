"""Posterior summaries on the final Plaza1 tree: Plaza1 end to end (run_plaza1.py's defaults, as scripts/sample_mmd.py), then
at n = 500 and 2000 posterior points:
  * device us of NFiSAM.posterior_summary(samples) -- every variable's mean, covariance and resultant length -- and of the
    same call with the 5 %, 50 %, 95 % quantiles, from HIP events around the whole call (20 replays after 5 warm-ups: median,
    min, max; the call uploads its tables and copies the results back, so host work between launches is inside the window),
  * wall us of the same calls, and of posterior_summary(n=n) (its own device draw) beside the walk alone
    (`samples` given as per-variable views makes the call assemble its matrix column range by column range first),
  * device us of the two C entries alone, tables uploaded, matrix in place (events around the launches only),
  * the baseline the run scripts use today: the device-to-host copy of the [n, total_dim] matrix, then per variable
    np.mean / scipy circmean and np.cov (wall us of the copy and of the loop, same replays),
  * the largest deviation of the device values from the float64 oracle of tests/test_sample_summary_cpu.py on this tree's
    points (first 60 variables) and the largest error / bound ratio on the GPU test's own table,
  * the compiler's resource figures of the unit (recorded below from its report).
Prints one JSON object.   usage: sample_summary.py [out.json]"""
import ctypes as C
import contextlib, io, json, os, sys, time
import numpy as np, torch
from scipy.stats import circmean
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from test_sample_summary_cpu import oracle_moments, oracle_quantiles

REPS, WARM = 20, 5
DEV = "cuda:0"
PROBS = [0.05, 0.5, 0.95]
# hipcc -O3 -ffp-contract=fast --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on sample_summary.hip
RESOURCES = dict(moments_mean_kernel=dict(vgprs=64, agprs=0, sgprs=59, scratch_bytes_per_lane=0, lds_bytes=96, waves_per_simd=8),
                 moments_cov_kernel=dict(vgprs=185, agprs=0, sgprs=106, scratch_bytes_per_lane=0, lds_bytes=0, waves_per_simd=2),
                 quantile_kernel=dict(vgprs=16, agprs=0, sgprs=52, scratch_bytes_per_lane=0, lds_bytes="8 x padded n (dynamic)",
                                      waves_per_simd=8))
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


def stats(ts):
    ts = np.asarray(ts[WARM:])
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
out = dict(dataset="Plaza1EFG", updates=len(steps), end_to_end_s=run_s, variables=len(order), total_dim=total_dim,
           columns=sum(v.dim for v in order), probs=PROBS, reps=REPS, warmups=WARM,
           stat="median / min / max of %d replays after %d warm-ups, us" % (REPS, WARM))
for n in (500, 2000):
    S = solver.posterior_launch(n)["S"]                              # [n, total_dim] on the device
    smp = {v: S[:, pcol[v]:pcol[v] + v.dim] for v in order}          # device views: what posterior_summary(samples) takes
    r = dict(matrix_bytes=int(S.numel() * 4))
    r["posterior_summary_device_us"], r["posterior_summary_wall_us"] = timed(lambda: solver.posterior_summary(samples=smp))
    r["with_quantiles_device_us"], r["with_quantiles_wall_us"] = timed(lambda: solver.posterior_summary(samples=smp, quantiles=PROBS))
    r["own_draw_device_us"], r["own_draw_wall_us"] = timed(lambda: solver.posterior_summary(n=n))
    r["walk_alone_device_us"], r["walk_alone_wall_us"] = timed(lambda: solver.posterior_launch(n))
    got = solver.posterior_summary(samples=smp, quantiles=PROBS, truth=truth)
    r["translation_rmse_m"] = got["translation_rmse"]

    # the two entries alone: tables uploaded, matrix in place
    cols = np.concatenate([np.arange(pcol[v], pcol[v] + v.dim) for v in order]).astype(np.int32)
    circ = np.concatenate([np.asarray(v.circular_dim_list, dtype=bool) for v in order]).astype(np.uint8)
    blocks = nh.pack_moment_blocks([v.dim for v in order])
    St = S.t().contiguous()
    probs = np.asarray(PROBS, dtype=np.float64)
    blk_d, cols_d, circ_d, probs_d = nh.upload(blocks.view(np.uint8).reshape(-1), cols, circ, probs, device=DEV, cached=True)
    ne, cov_count = int(cols.size), int((blocks["d"].astype(np.int64) ** 2).sum())
    mean = torch.empty(ne, dtype=torch.float64, device=DEV)
    res = torch.empty(ne, dtype=torch.float64, device=DEV)
    cov = torch.empty(cov_count, dtype=torch.float64, device=DEV)
    q = torch.empty(ne, len(PROBS), dtype=torch.float64, device=DEV)

    def moments_entry():
        nh._check(nh.lib().nfisam_sample_moments(nh._ptr(St), total_dim, n, blocks.ctypes.data_as(C.c_void_p),
                                                 C.c_void_p(blk_d.data_ptr()), len(order), nh._ptr(cols_d), ne, nh._ptr(circ_d), None,
                                                 nh._ptr(mean), nh._ptr(res), nh._ptr(cov), C.c_longlong(cov_count), nh._stream()),
                  "nfisam_sample_moments")

    def quantiles_entry():
        nh._check(nh.lib().nfisam_sample_quantiles(nh._ptr(St), total_dim, n, nh._ptr(cols_d), ne, nh._ptr(circ_d), nh._ptr(mean),
                                                   probs.ctypes.data_as(C.c_void_p), nh._ptr(probs_d), len(PROBS), nh._ptr(q),
                                                   nh._stream()), "nfisam_sample_quantiles")
    r["moments_entry_device_us"], _ = timed(moments_entry)
    r["quantiles_entry_device_us"], _ = timed(quantiles_entry)
    at, same, mean_h = 0, True, mean.cpu().numpy()
    for v in order:
        same &= bool(np.array_equal(mean_h[at:at + v.dim], got["mean"][v]))
        at += v.dim
    r["entries_equal_solver_call"] = same

    # the baseline: copy out, then the loop of the run scripts
    def copy_out():
        return S.cpu().numpy()

    def host_loop(H):
        res_ = {}
        for v in order:
            a = H[:, pcol[v]:pcol[v] + v.dim]
            m = a.mean(0)
            for k, c in enumerate(v.circular_dim_list):
                if c:
                    m[k] = circmean(a[:, k], high=np.pi, low=-np.pi)
            res_[v] = (m, np.cov(a, rowvar=False))
        return res_
    H = copy_out()
    _, r["d2h_copy_wall_us"] = timed(copy_out)
    _, r["numpy_scipy_loop_wall_us"] = timed(lambda: host_loop(H))
    r["host_total_over_device_call_wall"] = (r["d2h_copy_wall_us"]["median"] + r["numpy_scipy_loop_wall_us"]["median"]) / \
        r["posterior_summary_wall_us"]["median"]
    r["host_total_over_entry_device"] = (r["d2h_copy_wall_us"]["median"] + r["numpy_scipy_loop_wall_us"]["median"]) / \
        r["moments_entry_device_us"]["median"]

    # deviation from the float64 oracle on this tree's points
    worst = dict(mean_abs=0.0, cov_rel_to_s_e_s_f=0.0, resultant_abs=0.0, quantile_abs=0.0)
    for v in order[:60]:
        flags = [bool(c) for c in v.circular_dim_list]
        m_o, r_o, c_o, s = oracle_moments(H, list(range(pcol[v], pcol[v] + v.dim)), flags)
        worst["mean_abs"] = max(worst["mean_abs"], float(np.abs(got["mean"][v] - m_o).max()))
        worst["cov_rel_to_s_e_s_f"] = max(worst["cov_rel_to_s_e_s_f"], float((np.abs(got["cov"][v] - c_o) / np.outer(s, s)).max()))
        for k, c in enumerate(flags):
            if c:
                worst["resultant_abs"] = max(worst["resultant_abs"], abs(got["resultant"][v] - r_o[k]))
            want, _ = oracle_quantiles(H, pcol[v] + k, PROBS, c, got["mean"][v][k])
            worst["quantile_abs"] = max(worst["quantile_abs"], float(np.abs(got["quantiles"][v][:, k] - want).max()))
    r["largest_deviation_from_oracle_first_60_variables"] = worst
    print("n = %d: posterior_summary %.0f us device, %.0f us wall; host copy %.0f + loop %.0f us" % (
        n, r["posterior_summary_device_us"]["median"], r["posterior_summary_wall_us"]["median"], r["d2h_copy_wall_us"]["median"],
        r["numpy_scipy_loop_wall_us"]["median"]), flush=True)
    out["n%d" % n] = r

# error / bound on the GPU test's own table: every n of the test, with and without weights, and the quantile cases
import test_sample_summary_gpu as G
with contextlib.redirect_stdout(io.StringIO()):                     # (the tests print every figure)
    for weighted in (False, True):
        for n in G.NS:
            G.test_moments_match_the_float64_oracle(n, weighted)
    for n in G.NS + [127, 128, 129]:
        G.test_quantiles_match_numpy_on_the_sorted_keys(n)
out["largest_deviation"] = dict(error_over_bound_on_the_test_table=dict(G._worst),
                                rule="the bounds of tests/test_sample_summary_gpu.py (its docstring derives them)")
out["resources"] = RESOURCES
print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
