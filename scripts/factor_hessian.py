"""Hessian-vector products of the joint density (nfisam_factor_graph_hvp) on one MI355X:
  * the ratios |got - exact| / (2^-53 scale) against tests/golden/factor_hessian_exact.npz, largest per case, of the host
    formulas (`Factors.*.hess_x_log_pdf`) and of the device (every column of every block of the single-factor cases, the tables
    of tests/test_factor_hessian_gpu.py), and of the joint H v of the whole graphs; the tests' bound is C = 256;
  * device us of one H v launch (without and with the score output) next to one nfisam_factor_graph_score launch on the same
    table and points: the Plaza1 table (tests/data/Plaza1ADA0.4EFG), n = 500 and 2000 points = ground truth + 0.03 N(0, 1) per
    coordinate, a standard normal direction; HIP events around the C entries, tables uploaded, buffers in place, median of 20
    calls after one warm-up call;
  * the small range problem (tests/golden, the recipe of the GPU tests): `map_newton` at its defaults next to
    `map_refine(steps=20)` with the launches each made, and `laplace_approximation` at the Newton point.
No time, no ratio between the two launches and no gain is asserted.  Prints one JSON object.   usage: factor_hessian.py [out.json]"""
import json, os, random, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from test_factor_density_gpu import _case_table
from test_factor_exact_cpu import ratio
from test_factor_hessian_cpu import hessian_cases, hessian_fixture, hessian_graph, host_hessian

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


def columns(f, r):
    return np.concatenate([np.arange(r[v], r[v] + v.dim) for v in f.vars])


out = dict(what="Hessian-vector products of the joint density on one MI355X: scripts/factor_hessian.py",
           ratio_rule="largest |got - exact| / (2^-53 scale) over the unmasked entries; the tests' bound is C = 256")

# ---- the ratios of the tests ------------------------------------------------------------------------------------------------------
cases = hessian_cases()
host = {c.name: ratio(host_hessian(c)[c.mask], c.hess[c.mask], c.hess_scale[c.mask]) for c in cases}
single = [c for c in cases if len(c.factors) == 1]
terms, rows, total = _case_table([(c.cls, c.factors[0], c.x, None) for c in single])
gather = nh.pack_score_gather(terms, total)
n = 80
S = np.zeros((n, total), dtype=np.float32)
for c, r in zip(single, rows):
    S[:, columns(c.factors[0], r)] = c.x[np.arange(n) % c.x.shape[0]]
blocks = [np.zeros((n, c.x.shape[1], c.x.shape[1])) for c in single]
for k in range(max(c.x.shape[1] for c in single)):
    V = np.zeros((n, total))
    for c, r in zip(single, rows):
        if k < c.x.shape[1]:
            V[:, columns(c.factors[0], r)[k]] = 1.0
    H = nh.factor_graph_hvp(terms, S, V, DEV, gather=gather).cpu().numpy()
    for b, c, r in zip(blocks, single, rows):
        if k < c.x.shape[1]:
            b[:, :, k] = H[:, columns(c.factors[0], r)]
device = {}
for b, c in zip(blocks, single):
    idx = np.arange(n) % c.x.shape[0]
    m = c.mask[idx]
    device[c.name] = ratio(b[m], c.hess[idx][m], c.hess_scale[idx][m])
for kind, width in (("se2_prior", 3), ("se2_rel", 6)):                           # the sweeps: factor i at point i, its own slots
    sweep = [c for c in cases if c.name.startswith(kind) and len(c.factors) > 1]
    factors = [f for c in sweep for f in c.factors]
    tb = np.concatenate([nh.pack_factor_terms([f], {v: 3 * j for j, v in enumerate(f.vars)}) for f in factors])
    g = nh.pack_score_gather(tb, width)
    Sx = np.concatenate([c.x for c in sweep])
    bl = np.zeros((Sx.shape[0], width, width))
    for k in range(width):
        V = np.zeros(Sx.shape)
        V[:, k] = 1.0
        sl = nh.factor_graph_hvp(tb, Sx, V, DEV, gather=g, slots=True)[1].cpu().numpy()
        bl[:, :, k] = np.stack([sl[g["slot_off"][i]:g["slot_off"][i] + width, i] for i in range(Sx.shape[0])])
    off = 0
    for c in sweep:
        device[c.name] = ratio(bl[off:off + c.x.shape[0]], c.hess, c.hess_scale)
        off += c.x.shape[0]
out["cases"] = {c.name: dict(host=host[c.name], device=device[c.name]) for c in cases}
out["largest"] = dict(host=max(host.values()), device=max(device.values()))
hx = hessian_fixture()
graphs = {}
for key in ("ksd", "manhattan136"):
    factors, col, x, v, hv, scale = hessian_graph(hx, key)
    tb = nh.pack_factor_terms(factors, col)
    H = nh.factor_graph_hvp(tb, x, np.broadcast_to(v, x.shape), DEV).cpu().numpy()
    graphs[key] = dict(factors=len(factors), points=int(x.shape[0]), device=ratio(H, hv, scale))
out["graphs_joint_product"] = graphs
print("ratios:", out["largest"], graphs, flush=True)

# ---- one H v launch next to one score launch on the Plaza1 table -----------------------------------------------------------------
nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", "Plaza1ADA0.4EFG", "factor_graph.fg"), "fg",
                                          prior_cov_scale=0.1)
col, D = {}, 0
for v in nodes:
    col[v] = D
    D += v.dim
t = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
terms = nh.pack_factor_terms(factors, col)
gather = nh.pack_score_gather(terms, D)
nt, ns = int(terms.shape[0]), int(gather["n_slots"])
dev = nh._upload_named(DEV, terms=nh._table_bytes(terms), slot_off=gather["slot_off"], row_off=gather["row_off"], row_slot=gather["row_slot"])
timing = dict(reps=REPS, stat="median of %d calls after one warm-up call" % REPS, D=D, factors=nt, slots=ns)
rng = np.random.RandomState(0)
for n in (500, 2000):
    St = torch.from_numpy(np.ascontiguousarray((t + 0.03 * rng.randn(n, D)).astype(np.float32).T)).to(DEV)
    Vt = torch.from_numpy(np.ascontiguousarray(rng.randn(D, n))).to(DEV)
    Ht, Gt = torch.zeros(D, n, dtype=torch.float64, device=DEV), torch.zeros(D, n, dtype=torch.float64, device=DEV)
    scratch = torch.empty(2 * ns, n, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()

    def score():
        nh._check(nh.lib().nfisam_factor_graph_score(nh._ptr(dev["terms"]), nt, nh._ptr(St), D, n, nh._ptr(dev["slot_off"]), ns,
                                                     nh._ptr(dev["row_off"]), nh._ptr(dev["row_slot"]), nh._ptr(Gt),
                                                     nh._ptr(scratch), nh._stream()), "nfisam_factor_graph_score")

    def hvp(with_score):
        nh._check(nh.lib().nfisam_factor_graph_hvp(nh._ptr(dev["terms"]), nt, nh._ptr(St), nh._ptr(Vt), D, n,
                                                   nh._ptr(dev["slot_off"]), ns, nh._ptr(dev["row_off"]), nh._ptr(dev["row_slot"]),
                                                   nh._ptr(Ht), nh._ptr(Gt) if with_score else None, nh._ptr(scratch),
                                                   nh._stream()), "nfisam_factor_graph_hvp")
    q = dict(score_us=timed(score), hvp_us=timed(lambda: hvp(False)), hvp_with_score_us=timed(lambda: hvp(True)))
    q["hvp_over_score"] = q["hvp_us"] / q["score_us"]
    q["slot_mib_written_and_read"] = 2 * ns * n * 8 / 2 ** 20
    print("plaza1ada n = %d:" % n, q, flush=True)
    timing["n%d" % n] = q
out["timing_plaza1ada"] = timing

# ---- the small range problem --------------------------------------------------------------------------------------------------------
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
launches = {"n": 0}
for name in ("_hvp_launch", "_joint_launch", "_score_launch"):
    def counted(*a, _f=getattr(solver, name), **k):
        launches["n"] += 1
        return _f(*a, **k)
    setattr(solver, name, counted)
m = solver.map_newton(smp)
newton_calls, launches["n"] = launches["n"], 0
r = solver.map_refine(smp, steps=20)
refine_calls = launches["n"]
lap = solver.laplace_approximation(point=m["map_sample"])
out["small_range"] = dict(
    map_newton=dict(start_log_p=m["start_log_p"], log_p=m["log_p"], steps=m["steps"], entry_calls=newton_calls,
                    grad_norm=[float(g) for g in m["grad_norm"]], converged=[bool(c) for c in m["converged"]],
                    negative_curvature=[bool(c) for c in m["negative_curvature"]], climbers=[float(c) for c in m["climbers"]]),
    map_refine_20=dict(start_log_p=r["start_log_p"], log_p=r["log_p"], steps=r["steps"], entry_calls=refine_calls,
                       climbers=[float(c) for c in r["climbers"]]),
    laplace=dict(log_p=lap["log_p"], residual=lap["residual"], negative_curvature=lap["negative_curvature"],
                 sigma={v.name: [float(s) for s in np.sqrt(np.abs(np.diag(lap["cov"][v])))] for v in solver.elimination_ordering}))
print("small range:", out["small_range"], flush=True)

print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
