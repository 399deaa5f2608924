"""Stein variational direction and step (nfisam_sample_svgd, nfisam_sample_step) on one MI355X:
  * the deviations the GPU tests' bounds come from: the direction against the float64 numpy restatement of
    tests/test_sample_svgd_cpu.py at the shapes of tests/test_sample_svgd_gpu.py, largest |device - numpy| / (|numpy| + 1) per n,
    and the step fed the device's own phi (hist relative, points relative);
  * device us of one direction launch on the column layout of Plaza1-ADA (tests/data/Plaza1ADA0.4EFG), n = 500 and 2000
    points = ground truth + 0.03 N(0, 1) per coordinate standardised by their spread: one block per variable and one joint
    block, next to nfisam_sample_ksd on the same matrices (the joint block does comparable pair work in two passes), and of
    one step; HIP events around the calls, tables uploaded, matrices in place, median of 20 calls after one warm-up call;
  * the small range problem (tests/golden, the recipe of the GPU tests): `posterior_ksd` V-statistic and mean log p before
    and after `posterior_refine` at its defaults for the three kernels, and the gain of `map_refine` over `map_estimate`.
No time and no improvement is asserted.  Prints one JSON object.   usage: sample_svgd.py [out.json]"""
import json, os, random, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from test_sample_svgd_cpu import direction, step
from test_sample_svgd_gpu import _table_case, deviation

REPS = 20
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")


def timed(call, reps=REPS):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps + 1):
        ev0.record()
        call()
        ev1.record()
        ev1.synchronize()
        ts.append(ev0.elapsed_time(ev1) * 1e3)
    return float(np.median(ts[1:]))


out = dict(what="Stein variational direction and step on one MI355X: scripts/sample_svgd.py, and the deviations the GPU tests' "
                "bounds are 16 x of", deviation_rule="largest |device - numpy| / (|numpy| + 1); the test bound is 16 x the largest")

# ---- the deviations of the tests --------------------------------------------------------------------------------------------------
dev_n = {}
for n in (1, 2, 63, 64, 65, 130):
    x, xw, s, table, cols, scale, scale0, wrap = _table_case(n, 100 * n)
    dev_n["n%d" % n] = max(deviation(nh.svgd_direction(p, s, table, cols, scale=sc, wrap=wr, device=DEV).cpu().numpy(),
                                     direction(p, s, table, cols, sc, wr))
                           for p, sc, wr in ((x, None, None), (xw, scale, wrap), (x, scale0, None), (xw, scale0, wrap)))
out["direction_vs_numpy_restatement"] = dev_n
n = 130
x, xw, s, table, cols, scale, scale0, wrap = _table_case(n, 55, widths=(3, 16, 1))
rng = np.random.RandomState(8)
eps, hist0 = rng.uniform(1e-3, 0.5, cols.size), rng.uniform(0.1, 100.0, (cols.size, n))
Xt = torch.from_numpy(np.ascontiguousarray(xw.T)).to(DEV)
Phi = nh.svgd_direction_t(Xt, torch.from_numpy(np.ascontiguousarray(s.T)).to(DEV), table, cols, scale=scale, wrap=wrap)
hist = torch.from_numpy(hist0).to(DEV)
nh.sample_step_t(Xt, cols, Phi, hist, eps, wrap=wrap)
want_x, want_h = step(xw, cols, Phi.cpu().numpy(), hist0, eps, wrap)
got_x = Xt.cpu().numpy().T.astype(np.float64)
out["step_vs_numpy_restatement"] = dict(hist_relative=float(np.max(np.abs(hist.cpu().numpy() - want_h) / want_h)),
                                        points_relative=float(np.max(np.abs(got_x - want_x) / np.maximum(np.abs(want_x), 1e-30))),
                                        float32_ulp=2.0 ** -23)
print("deviations:", out["direction_vs_numpy_restatement"], out["step_vs_numpy_restatement"], flush=True)

# ---- one direction launch on the Plaza1 column layout ---------------------------------------------------------------------------
nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", "Plaza1ADA0.4EFG", "factor_graph.fg"), "fg",
                                          prior_cov_scale=0.1)
col, D = {}, 0
for v in nodes:
    col[v] = D
    D += v.dim
circ = np.concatenate([[bool(c) for c in v.circular_dim_list] for v in nodes]).astype(np.uint8)
t = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
terms = nh.pack_factor_terms(factors, col)
gather = nh.pack_score_gather(terms, D)
timing = dict(reps=REPS, stat="median of %d calls after one warm-up call" % REPS, D=D, variables=len(nodes))
rng = np.random.RandomState(0)
for n in (500, 2000):
    x = (t + 0.03 * rng.randn(n, D)).astype(np.float32)
    St = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    Gt = nh.factor_graph_score_t(terms, St, DEV, gather=gather)
    scale = 1.0 / x.astype(np.float64).std(0)
    q = dict(tiles=((n + 63) // 64) ** 2)
    for name, dims in (("per_variable", [v.dim for v in nodes]), ("joint", [D])):
        table = nh.pack_mmd_blocks(dims, np.sqrt(np.asarray(dims, dtype=np.float64)))
        tables = nh.svgd_tables(DEV, table, np.arange(D), scale, circ, np.full(D, 1e-3))
        count = int(nh.lib().nfisam_sample_svgd_scratch_count(n, len(dims), D))
        scratch = torch.empty(count, dtype=torch.float64, device=DEV)
        Phi = torch.zeros(D, n, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()

        def svgd():
            nh._check(nh.lib().nfisam_sample_svgd(nh._ptr(St), D, n, nh._ptr(Gt), tables["host"].ctypes.data_as(nh.C.c_void_p),
                                                  nh._ptr(tables["blocks"]), len(dims), nh._ptr(tables["cols"]), D,
                                                  nh._ptr(tables["scale"]), nh._ptr(tables["wrap"]), nh._ptr(Phi), nh._ptr(scratch),
                                                  nh._stream()), "nfisam_sample_svgd")
        q[name] = dict(blocks=len(dims), groups=q["tiles"] * len(dims), scratch_mib=count * 8 / 2 ** 20, direction_us=timed(svgd))
        q[name]["ps_per_pair_column"] = q[name]["direction_us"] * 1e6 / (n * n * D)
        if name == "joint":
            hist = torch.zeros(D, n, dtype=torch.float64, device=DEV)
            work = St.clone()
            q["step_us"] = timed(lambda: nh.sample_step_t(work, None, Phi, hist, None, checked=True, tables=tables))
        del scratch
    precision = scale * scale / D
    nh.ksd_sums_t(St, Gt, precision, wrap=circ)
    pd, wd = nh._upload_named(DEV, p=precision, w=circ).values()
    ks = torch.empty(int(nh.lib().nfisam_sample_ksd_scratch_count(n)), dtype=torch.float64, device=DEV)
    row, diag = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.float64, device=DEV)
    q["ksd_us"] = timed(lambda: nh._check(nh.lib().nfisam_sample_ksd(nh._ptr(St), nh._ptr(Gt), D, n, nh._ptr(pd), nh._ptr(wd),
                                                                     nh._ptr(row), nh._ptr(diag), None, nh._ptr(ks), nh._stream()),
                                          "nfisam_sample_ksd"))
    q["joint_over_ksd"] = q["joint"]["direction_us"] / q["ksd_us"]
    print("plaza1ada n = %d:" % n, q, flush=True)
    timing["n%d" % n] = q
    del St, Gt, Phi, ks
    torch.cuda.empty_cache()
out["timing_plaza1ada"] = timing

# ---- the small range problem: what the refinement does to the trained posterior's draw ---------------------------------------------------
from slam.NFiSAM import NFiSAM, NFiSAMArgs
fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
kwargs = json.loads(str(fx["arguments"]))
kwargs["cuda_training"] = True
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "factor_graph.fg")
    with open(path, "w") as f:
        f.write(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    nodes, truth, factors = graph_file_parser(path, "fg", prior_cov_scale=0.1)
steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))
solver = NFiSAM(NFiSAMArgs(**kwargs))
for vs, fs in steps:
    for v in vs: solver.add_node(v)
    for f in fs: solver.add_factor(f)
    solver.update_physical_and_working_graphs()
    smp = solver.incremental_inference()
smp = {v: np.array(smp[v]) for v in solver.elimination_ordering}
before = solver.posterior_ksd(smp)
small = dict(n=before["n"], before=dict(vstat=before["vstat"], ustat=before["ustat"], mean_log_p=float(solver.joint_log_pdf(smp).mean())))
for kernel in ("variable", "joint", None):
    r = solver.posterior_refine(smp, kernel=kernel)
    k = solver.posterior_ksd(r["samples"])
    small["after_%s" % kernel] = dict(steps=r["steps"], vstat=k["vstat"], ustat=k["ustat"], mean_log_p=float(r["log_p_after"].mean()),
                                      min_log_p=float(r["log_p_after"].min()))
    print("small range, kernel = %r:" % (kernel,), small["after_%s" % kernel], "before:", small["before"], flush=True)
m = solver.map_refine(smp)
small["map_refine"] = dict(start_log_p=m["start_log_p"], log_p=m["log_p"], gain=m["log_p"] - m["start_log_p"], improved=m["improved"],
                           climbers=[float(c) for c in m["climbers"]], steps=m["steps"], top=m["top"])
print("small range, map_refine:", small["map_refine"], flush=True)
out["small_range"] = small

print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
