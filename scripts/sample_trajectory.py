"""Trajectory error per posterior sample on the final Plaza1 tree: Plaza1 end to end (run_plaza1.py's defaults, as
scripts/sample_summary.py), then at n = 500 and 2000 posterior points:
  * device us of NFiSAM.posterior_trajectory_error(samples) -- every sample aligned and graded, RPE at strides 1 and 10, the
    posterior mean graded the reference's way -- from HIP events around the whole call (20 replays after 5 warm-ups: median,
    min, max; the call uploads its tables and copies the results back, so host work between launches is inside the window),
    and its wall us,
  * device us of the two C entries alone, tables uploaded, matrix in place (events around the launches only),
  * the baseline, what a run script would do today: the device-to-host copy of the [n, total_dim] matrix, then a numpy loop
    that calls utils.Functions.kabsch_umeyama per sample and forms its RMSE (wall us of the copy and of the loop, same
    replays), and the ratio of the two,
  * the largest error / bound of the device values against the float64 oracle of tests/test_sample_trajectory_cpu.py on
    this tree's points (first 100 samples), and on the GPU tests' own tables,
  * the aligned and unaligned ATE distribution of the run, and the posterior mean's ATE beside it,
  * the compiler's resource figures of the unit (recorded below from its report).
Prints one JSON object.   usage: sample_trajectory.py [out.json]"""
import ctypes as C
import contextlib, io, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from utils import Functions as FN
from test_sample_trajectory_cpu import bounds, oracle_trajectory

REPS, WARM = 20, 5
DEV = "cuda:0"
STRIDES = (1, 10)
# hipcc -O3 -ffp-contract=fast --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on sample_trajectory.hip
RESOURCES = dict(traj_error_kernel=dict(vgprs=58, agprs=0, sgprs=57, scratch_bytes_per_lane=0, lds_bytes=10240, waves_per_simd=8),
                 traj_entry_reduce_kernel=dict(vgprs=8, agprs=0, sgprs=14, scratch_bytes_per_lane=0, lds_bytes=0, waves_per_simd=8),
                 traj_rpe_kernel=dict(vgprs=58, agprs=0, sgprs=104, scratch_bytes_per_lane=0, lds_bytes=4096, waves_per_simd=7))
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


def dist(a):
    q = np.quantile(a, [0.05, 0.5, 0.95])
    return dict(min=float(a.min()), q05=float(q[0]), median=float(q[1]), q95=float(q[2]), max=float(a.max()), mean=float(a.mean()))


order = list(solver.elimination_ordering)
pcol, total_dim = solver._post_columns()
poses = [v for v in solver.physical_vars if v.dim == 3 and v.circular_dim_list[2] and v in truth]
lands = [v for v in solver.physical_vars if v.dim == 2 and v in truth]
every = poses + lands
P = len(poses)
out = dict(dataset="Plaza1EFG", updates=len(steps), end_to_end_s=run_s, variables=len(order), total_dim=total_dim, poses=P,
           landmarks=len(lands), strides=list(STRIDES), reps=REPS, warmups=WARM,
           stat="median / min / max of %d replays after %d warm-ups, us" % (REPS, WARM))
truth64 = [np.asarray(truth[v], dtype=np.float64) for v in every]
entries = nh.pack_traj_entries([pcol[v] for v in every], [pcol[v] + 1 for v in every],
                               [pcol[v] + 2 if k < P else -1 for k, v in enumerate(every)], np.array([a[:2] for a in truth64]),
                               [a[2] if a.size > 2 else 0.0 for a in truth64], landmark=np.arange(len(every)) >= P)
pairs = nh.pack_traj_pairs(np.arange(P), STRIDES)
A = np.array([a[:2] for a in truth64])[:P]
for n in (500, 2000):
    S = solver.posterior_launch(n)["S"]                              # [n, total_dim] on the device
    smp = {v: S[:, pcol[v]:pcol[v] + v.dim] for v in order}          # device views: what the solver call takes
    r = dict(matrix_bytes=int(S.numel() * 4))
    call = lambda align="rigid": solver.posterior_trajectory_error(truth, samples=smp, align=align, strides=STRIDES, threshold=1.0)   # noqa: E731
    r["posterior_trajectory_error_device_us"], r["posterior_trajectory_error_wall_us"] = timed(call)
    got, plain = call(), call("none")
    r["ate_aligned_m"], r["ate_unaligned_m"] = dist(got["ate"]), dist(plain["ate"])
    r["landmark_rmse_aligned_m"] = dist(got["landmark_rmse"]) if lands else None
    r["heading_rms_aligned_rad"] = dist(got["heading_rms"])
    r["rpe"] = {str(k): dict(trans_m=dist(v["trans"]), rot_rad=dist(v["rot"])) for k, v in got["rpe"].items()}
    r["mean_trajectory_ate_m"] = dict(aligned=got["mean_trajectory"]["ate"], unaligned=plain["mean_trajectory"]["ate"])
    r["share_of_samples_below_1m_aligned"] = got["summary"]["below"]
    worst_var = max(got["per_pose_rmse"], key=got["per_pose_rmse"].get)
    r["worst_variable"] = dict(name=worst_var.name, rmse_m=got["per_pose_rmse"][worst_var])

    # the two entries alone: tables uploaded, matrix in place
    St = S.t().contiguous()
    ent_d, pairs_d = nh.upload(entries.view(np.uint8).reshape(-1), pairs.view(np.uint8).reshape(-1), device=DEV, cached=True)
    o8 = torch.empty(nh.TRAJ_OUT_ROWS, n, dtype=torch.float64, device=DEV)
    i2 = torch.empty(2, n, dtype=torch.int32, device=DEV)
    sums = torch.empty(len(every) + 1, dtype=torch.float64, device=DEV)
    scratch = torch.empty(int(nh.lib().nfisam_sample_trajectory_scratch_count(n, len(every))), dtype=torch.float64, device=DEV)
    rp = torch.empty(len(STRIDES), 2, n, dtype=torch.float64, device=DEV)

    def error_entry():
        nh._check(nh.lib().nfisam_sample_trajectory_error(nh._ptr(St), total_dim, n, entries.ctypes.data_as(C.c_void_p), nh._ptr(ent_d),
                                                          len(every), 1, 0, None, nh._ptr(o8), nh._ptr(i2), nh._ptr(sums),
                                                          nh._ptr(scratch), nh._stream()), "nfisam_sample_trajectory_error")

    def rpe_entry():
        nh._check(nh.lib().nfisam_sample_trajectory_rpe(nh._ptr(St), total_dim, n, entries.ctypes.data_as(C.c_void_p), nh._ptr(ent_d),
                                                        len(every), pairs.ctypes.data_as(C.c_void_p), nh._ptr(pairs_d), int(pairs.size),
                                                        len(STRIDES), nh._ptr(rp), nh._stream()), "nfisam_sample_trajectory_rpe")
    r["error_entry_device_us"], _ = timed(error_entry)
    r["rpe_entry_device_us"], _ = timed(rpe_entry)
    r["entries_equal_solver_call"] = bool(np.array_equal(np.sqrt(o8[4].cpu().numpy() / P), got["ate"]))

    # the baseline: copy out, then a numpy loop of n SVD fits
    def copy_out():
        return S.cpu().numpy()

    xy_cols = np.array([[pcol[v], pcol[v] + 1] for v in poses])

    def host_loop(H):
        ate = np.empty(H.shape[0])
        for i in range(H.shape[0]):
            B = H[i][xy_cols].astype(np.float64)
            R, _, _ = FN.kabsch_umeyama(A, B)
            t = A.mean(0) - R @ B.mean(0)
            ate[i] = np.sqrt(np.mean(np.sum((A - (B @ R.T + t)) ** 2, axis=1)))
        return ate
    H = copy_out()
    _, r["d2h_copy_wall_us"] = timed(copy_out)
    _, r["numpy_kabsch_loop_wall_us"] = timed(lambda: host_loop(H))
    host = r["d2h_copy_wall_us"]["median"] + r["numpy_kabsch_loop_wall_us"]["median"]
    r["host_total_over_solver_call_wall"] = host / r["posterior_trajectory_error_wall_us"]["median"]
    r["host_total_over_error_entry_device"] = host / r["error_entry_device_us"]["median"]
    r["host_loop_ate_minus_device_max_abs_m"] = float(np.abs(host_loop(H) - got["ate"]).max())

    # error / bound against the float64 oracle on this tree's points
    m = min(n, 100)
    o = oracle_trajectory(H[:m], entries, "rigid")
    b = bounds(o, entries)
    want = np.sqrt(o["sse_traj"] / P)
    r["largest_error_over_bound_first_100_samples"] = dict(
        ate=float((np.abs(got["ate"][:m] - want) / (b["resid"] + b["rel"] * want)).max()),
        theta=float((np.abs((got["theta"][:m] - o["theta"] + np.pi) % (2 * np.pi) - np.pi) / b["theta"]).max()),
        t=float((np.abs(got["t"][:m] - o["t"]).max(axis=1) / b["t"]).max()),
        largest_ate_bound_m=float((b["resid"] + b["rel"] * want).max()), smallest_kappa=float(o["kappa"].min()))
    print("n = %d: posterior_trajectory_error %.0f us device, %.0f us wall; entries %.0f + %.0f us; host copy %.0f + loop %.0f us" % (
        n, r["posterior_trajectory_error_device_us"]["median"], r["posterior_trajectory_error_wall_us"]["median"],
        r["error_entry_device_us"]["median"], r["rpe_entry_device_us"]["median"], r["d2h_copy_wall_us"]["median"],
        r["numpy_kabsch_loop_wall_us"]["median"]), flush=True)
    out["n%d" % n] = r

# error / bound on the GPU tests' own tables
import test_sample_trajectory_gpu as G
with contextlib.redirect_stdout(io.StringIO()):                     # (the tests print every figure)
    for n in G.NS:
        for P_ in G.PS:
            G.test_errors_match_the_float64_oracle(n, P_)
            if P_ > 1:
                G.test_relative_pose_error_matches_the_oracle(n, P_)
    for P_ in (4, 64, 257):
        G.test_a_mirrored_sample_with_reflect_off_and_on(P_)
    G.test_ill_conditioned_fits_against_mpmath()
out["largest_ratio"] = dict(error_over_bound_on_the_test_tables=dict(G._worst),
                            rule="the bounds of tests/test_sample_trajectory_gpu.py (its docstring derives them)")
out["resources"] = RESOURCES
print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
