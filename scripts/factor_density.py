"""Joint log-density of the factor graph on the final Plaza1 tree: Plaza1 end to end (run_plaza1.py's defaults, as
scripts/posterior_density.py), then at n = 500 and n = 10 000 posterior samples
  * device us of nfisam_factor_graph_log_density from HIP events around the launch (table uploaded, sample matrix assembled;
    median of 20 calls after one warm-up call),
  * wall us of NFiSAM.joint_log_pdf(samples) and of NFiSAM.posterior_diagnostics(samples),
  * the baseline: the numpy `Factors.log_pdf` loop over the same factors on the CPU (median of 3),
  * the deviation of the device terms from that loop,
and, on the fixture tests/golden/factor_density.npz, the device-vs-reference deviation the GPU tests' bounds are 16 x of.
Prints one JSON object.   usage: factor_density.py [out.json]
                                 factor_density.py --trace-only    (no solver run: 5 calls per n on Plaza1's graph at ground truth
                                                                    + noise; the target of rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT)
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally

REPS = 20
DEV = "cuda:0"
np.random.seed(0); torch.manual_seed(0)
nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", "Plaza1EFG", "factor_graph.fg"), "fg")


def device_call(terms_dev, nt, St, log_p, per):
    total_dim, n = St.shape
    nh._check(nh.lib().nfisam_factor_graph_log_density(C.c_void_p(terms_dev.data_ptr()), nt, nh._ptr(St), int(total_dim), int(n),
                                                       nh._ptr(log_p), nh._ptr(per), nh._stream()), "nfisam_factor_graph_log_density")


if "--trace-only" in sys.argv:
    col, off = {}, 0
    for v in nodes:
        col[v] = off
        off += v.dim
    terms = nh.pack_factor_terms(factors, col)
    nh.check_factor_terms(terms, off)
    terms_dev, = nh.upload(terms.view(np.uint8).reshape(-1), device=DEV, cached=True)
    t = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
    for n in (500, 10000):
        St = torch.from_numpy(np.ascontiguousarray((t + 0.03 * np.random.randn(n, off)).T, dtype=np.float32)).to(DEV)
        log_p = torch.empty(n, dtype=torch.float64, device=DEV)
        per = torch.empty(len(factors), n, dtype=torch.float64, device=DEV)
        for _ in range(5):
            device_call(terms_dev, len(factors), St, log_p, per)
        torch.cuda.synchronize()
        print("n = %d: %d factors, 5 calls, finite: %s" % (n, len(factors), bool(torch.isfinite(log_p).all())))
    sys.exit(0)

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


def median_after_first(f, reps=REPS):
    ts = [f() for _ in range(reps + 1)]
    return float(np.median(ts[1:]))


facs = solver.physical_factors
out = dict(dataset="Plaza1EFG", updates=len(steps), end_to_end_s=run_s, variables=len(solver.physical_vars), factors=len(facs),
           factor_classes={k: sum(f.__class__.__name__ == k for f in facs) for k in sorted({f.__class__.__name__ for f in facs})},
           reps=REPS, stat="median of %d calls after one warm-up call" % REPS,
           tree_density_us_for_comparison={"n500": 66.7, "n10000": 708})
pcol, total_dim = solver._post_columns()
cache = solver._joint_terms(pcol)
terms_dev, = nh.upload(cache["terms"].view(np.uint8).reshape(-1), device=DEV, cached=True)
for n in (500, 10000):
    solver._args.posterior_sample_num = n
    smp = solver.sample_posterior()
    lp = solver.joint_log_pdf(smp)
    d = solver.posterior_diagnostics(smp)
    r = dict(finite=bool(np.all(np.isfinite(lp))), mean_log_p=float(lp.mean()), elbo=d["elbo"], log_evidence=d["log_evidence"],
             ess=d["ess"], map_index=d["map_index"], max_log_p=float(lp.max()))

    def wall_joint():
        a = time.perf_counter()
        solver.joint_log_pdf(smp)
        return (time.perf_counter() - a) * 1e6

    def wall_diag():
        a = time.perf_counter()
        solver.posterior_diagnostics(smp)
        return (time.perf_counter() - a) * 1e6
    r["joint_log_pdf_wall_us"] = median_after_first(wall_joint)
    r["posterior_diagnostics_wall_us"] = median_after_first(wall_diag)
    S = np.zeros((n, total_dim), dtype=np.float32)
    for v in solver.elimination_ordering:
        S[:, pcol[v]:pcol[v] + v.dim] = smp[v]
    St = torch.from_numpy(np.ascontiguousarray(S.T)).to(DEV)
    log_p = torch.empty(n, dtype=torch.float64, device=DEV)
    per = torch.empty(len(facs), n, dtype=torch.float64, device=DEV)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def kernel():
        ev0.record()
        device_call(terms_dev, len(facs), St, log_p, per)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3
    r["kernel_us"] = median_after_first(kernel)
    r["kernel_equals_solver_call"] = bool(np.array_equal(log_p.cpu().numpy(), lp))
    S64 = S.astype(np.float64)

    def host():
        a = time.perf_counter()
        tot = np.zeros(n)
        for f in facs:
            tot = tot + f.log_pdf(np.concatenate([S64[:, pcol[v]:pcol[v] + v.dim] for v in f.vars], 1))
        host.total = tot
        return (time.perf_counter() - a) * 1e6
    r["numpy_loop_wall_us"] = median_after_first(host, 3)
    r["max_abs_diff_vs_numpy_over_abs_plus_1"] = float(np.max(np.abs(host.total - lp) / (np.abs(lp) + 1)))
    r["speedup_vs_numpy_kernel"] = r["numpy_loop_wall_us"] / r["kernel_us"]
    r["speedup_vs_numpy_wall"] = r["numpy_loop_wall_us"] / r["joint_log_pdf_wall_us"]
    out["n%d" % n] = r

# the deviation the GPU tests' bounds come from: device vs the reference's values, every value of the fixture
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_factor_density_cpu as T
import test_factor_density_gpu as G
fx = T.fixture()
cases = T.part_a_cases(fx)
terms, rows, total = G._case_table(cases)
worst = 0.0
for n in G.NS:
    S, ref = G._case_points(cases, rows, total, n)
    per = nh.factor_graph_log_density(terms, S, DEV, per_factor=True)[1].cpu().numpy()
    worst = max(worst, float(np.max(np.abs(per - ref) / (np.abs(ref) + 1))))
dev = {"part_a": worst}
for key in sorted(T.GRAPHS):
    terms, _, _, x, terms_ref, total_ref = G._graph_table(key)
    lp, per = nh.factor_graph_log_density(terms, x, DEV, per_factor=True)
    dev[key + "_terms"] = float(np.max(np.abs(per.cpu().numpy() - terms_ref) / (np.abs(terms_ref) + 1)))
    dev[key + "_total"] = float(np.max(np.abs(lp.cpu().numpy() - total_ref) / (np.abs(total_ref) + 1)))
out["device_vs_reference_max_abs_diff_over_abs_plus_1"] = dev
out["test_bounds"] = dict(rtol_atol_part_a=G.RTOL_A, rtol_atol_graphs=G.RTOL_G, rule="16 x the measured deviation")
print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
