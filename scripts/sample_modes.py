"""Posterior modes on a final tree: a dataset end to end (run_plaza1.py's defaults, as scripts/sample_summary.py), then at
n = 500 and 2000 posterior points:
  * device us of NFiSAM.posterior_modes(samples) -- every variable's modes, masses and labels -- from HIP events around the
    whole call (20 replays after 5 warm-ups at n = 500, 5 after 2 at n = 2000: median, min, max; the call computes the columns' spreads, uploads its tables and
    copies the mode tables back, so host work between launches is inside the window), and its wall us,
  * wall us of posterior_modes(n=n) (its own device draw) beside the walk alone: how much of the call is the walk,
  * device us of both launches: the C entry alone (ascent and merge between one pair of events; matrix in place, outputs
    allocated, scales given), the merge launch alone on the same converged points (nfisam_sample_modes_merge), the ascent as
    their difference; and the entry stopped after one shift (tol = 1e30: two passes of the ascent, for the fixed cost),
  * how many variables hold more than one mode, the most iterations an ascent took, ascents that did not converge,
  * the largest deviation of the device's converged points and densities from the float64 oracle of
    tests/test_sample_modes_cpu.py on this tree's points (first 12 variables, n = 500), as error / bound of
    tests/test_sample_modes_gpu.py,
  * with --tests: the largest error / bound ratio over the GPU test's own cases,
  * the compiler's resource figures of the unit (recorded below from its report).
Prints one JSON object and merges it under the dataset's name into out.json.
usage: sample_modes.py [--tests] [--updates=K (default: all)] [dataset (default Plaza1EFG)] [out.json]"""
import contextlib, io, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from utils import Statistics as ST
from test_sample_modes_cpu import oracle_ascent, wrap_pi

REPS, WARM = 20, 5
DEV = "cuda:0"
# hipcc -O3 -ffp-contract=fast --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on sample_modes.hip
RESOURCES = dict(modes_ascent_kernel=dict(vgprs=218, agprs=0, sgprs=106, sgpr_spills_to_vgpr_lanes=73, scratch_bytes_per_lane=0,
                                          lds_bytes=52704, waves_per_simd=2),
                 modes_merge_kernel=dict(vgprs=40, agprs=0, sgprs=86, scratch_bytes_per_lane=0, lds_bytes=4880, waves_per_simd=8))
flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
dataset = args[0] if args else "Plaza1EFG"
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
out = dict(dataset=dataset, updates=len(steps), updates_of_the_dataset=all_updates, end_to_end_s=run_s, variables=len(order), total_dim=total_dim, reps=REPS,
           warmups=WARM, stat="median / min / max of the replays after the warm-ups that every n records, us",
           arguments=dict(tol=1e-7, merge=1e-2, max_iters=500, max_modes=16, sigma="Scott's rule on standardised columns"))
for n in (500, 2000):
    if n == 2000:
        REPS, WARM = 5, 2                                            # (16 x the pair work per call)
    S = solver.posterior_launch(n)["S"]                              # [n, total_dim] on the device
    smp = {v: S[:, pcol[v]:pcol[v] + v.dim] for v in order}          # device views: what posterior_modes(samples) takes
    r = dict(matrix_bytes=int(S.numel() * 4), reps=REPS, warmups=WARM)
    r["posterior_modes_device_us"], r["posterior_modes_wall_us"] = timed(lambda: solver.posterior_modes(samples=smp))
    r["own_draw_device_us"], r["own_draw_wall_us"] = timed(lambda: solver.posterior_modes(n=n))
    r["walk_alone_device_us"], r["walk_alone_wall_us"] = timed(lambda: solver.posterior_launch(n))
    r["walk_share_of_own_draw_wall"] = r["walk_alone_wall_us"]["median"] / r["own_draw_wall_us"]["median"]
    got = solver.posterior_modes(samples=smp)
    counts = np.array([len(got["modes"][v]) for v in order])
    r["variables_with_more_than_one_mode"] = int((counts > 1).sum())
    r["most_modes_of_a_variable"] = int(counts.max())
    r["ascents_not_converged"] = int(sum(got["not_converged"].values()))
    r["unlabelled"] = int(sum(got["unlabelled"].values()))

    # the entry alone: matrix in place, outputs allocated, the same scales and bandwidths
    St = S.t().contiguous()
    cols = np.concatenate([np.arange(pcol[v], pcol[v] + v.dim) for v in order]).astype(np.int32)
    circ = np.zeros(total_dim, dtype=bool)
    for v in order:
        circ[pcol[v]:pcol[v] + v.dim] = [bool(c) for c in v.circular_dim_list]
    res = ST.sample_modes_t(St, [np.arange(pcol[v], pcol[v] + v.dim) for v in order], circular=circ)
    r["most_iterations_of_an_ascent"] = int(res["iterations"]["max"].max())
    table = nh.pack_mmd_blocks([v.dim for v in order], res["sigma"])
    scale, wrap = res["scale"][cols], circ[cols].astype(np.uint8)
    buf = res["raw"]
    r["entry_device_us"], _ = timed(lambda: nh.sample_modes_t(St, table, cols, scale, wrap, checked=True, out=buf))
    r["merge_launch_device_us"], _ = timed(lambda: nh.sample_modes_merge_t(buf, total_dim, table, cols, scale, wrap, checked=True))
    r["ascent_launch_device_us_by_difference"] = r["entry_device_us"]["median"] - r["merge_launch_device_us"]["median"]
    r["entry_one_shift_device_us"], _ = timed(lambda: nh.sample_modes_t(St, table, cols, scale, wrap, tol=1e30, checked=True, out=buf))
    again = nh.sample_modes_t(St, table, cols, scale, wrap, checked=True)
    r["entry_equals_solver_call"] = bool(all(
        np.array_equal(again["mode_pos"][b, :len(got["modes"][v]), :v.dim].cpu().numpy(), np.array([m["position"] for m in got["modes"][v]]))
        for b, v in enumerate(order)))
    kernel_evals = float(np.abs(again["iters"].cpu().numpy().astype(np.int64)).sum() + len(order) * n) * n
    r["float64_kernel_evaluations"] = kernel_evals
    r["kernel_evaluations_per_us"] = kernel_evals / r["entry_device_us"]["median"]

    if n == 500:                                                     # deviation from the float64 oracle on this tree's points
        H, pos_d, dens_d, it_d = S.cpu().numpy(), again["pos"].cpu().numpy(), again["dens"].cpu().numpy(), again["iters"].cpu().numpy()
        worst, differ, at = dict(position_error_over_bound=0.0, density_error_over_bound=0.0), 0, 0
        for b, v in enumerate(order[:12]):
            c = list(range(pcol[v], pcol[v] + v.dim))
            fl = [bool(f) for f in v.circular_dim_list]
            sc, inv = res["scale"][c], 1.0 / (2.0 * res["sigma"][b] ** 2)
            pos, dens, it = oracle_ascent(H, c, fl, sc, inv)
            same = it == it_d[b]
            differ += int((~same).sum())
            diff = pos_d[at:at + v.dim].T - pos
            diff[:, fl] = wrap_pi(diff[:, fl])
            Sc = np.abs(H[:, c].astype(np.float64) * sc).max()
            worst["position_error_over_bound"] = max(worst["position_error_over_bound"],
                                                     float((np.abs(diff * sc)[same] / (1e-12 * (1 + Sc))).max()))
            worst["density_error_over_bound"] = max(worst["density_error_over_bound"],
                                                    float((np.abs(dens_d[b] - dens)[same] / (1e-11 * dens[same])).max()))
            at += v.dim
        worst["starts_whose_iteration_count_differs"] = differ
        worst["starts"] = 12 * n
        r["largest_deviation_from_oracle_first_12_variables"] = worst
    print("n = %d: posterior_modes %.0f us device, %.0f us wall; entry %.0f us; %d of %d variables multi-modal" % (
        n, r["posterior_modes_device_us"]["median"], r["posterior_modes_wall_us"]["median"], r["entry_device_us"]["median"],
        r["variables_with_more_than_one_mode"], len(order)), flush=True)
    out["n%d" % n] = r

if "--tests" in flags:                                              # error / bound over the GPU test's own cases
    import test_sample_modes_gpu as G
    with contextlib.redirect_stdout(io.StringIO()):                 # (the tests print every figure)
        for it in (1, 8, 30):
            for n in (1, 63, 65, 200):
                G.test_fixed_count_matches_the_oracle(n, it)
            G.test_fixed_count_on_wide_narrow_repeated_and_unscaled_blocks(it)
            G.test_fixed_count_with_zero_weights_and_a_start_out_of_reach(it)
        for n, seed in ((65, 5), (65, 6), (65, 7), (200, 5), (200, 6), (200, 7)):
            G.test_stopping_and_merge_equal_the_oracle(n, seed)
        G.test_stopping_and_merge_with_weights()
    out["largest_ratio"] = dict(error_over_bound_in_the_gpu_tests=dict(G._worst),
                                rule="the bounds of tests/test_sample_modes_gpu.py (its docstring states them)")
out["resources"] = RESOURCES
print(json.dumps(out))
if len(args) > 1:
    doc = {}
    if os.path.exists(args[1]):
        with open(args[1]) as f:
            doc = json.load(f)
    doc[dataset] = out
    with open(args[1], "w") as f:
        json.dump(doc, f, indent=1)
