"""The Metropolis kernels (nfisam_sample_propose, nfisam_sample_accept) on one MI355X:
  * how far the device lies from the float64 numpy restatement of tests/test_sample_mcmc_cpu.py at the shapes of
    tests/test_sample_mcmc_gpu.py: the largest |proposal - restatement| in float32 ulp and the largest |log alpha - restatement|
    as a fraction of the tests' summation bound B (the bounds are derived, not measured: these are for the record);
  * device us of the propose + accept pair on the column layouts of Plaza1 (tests/data/Plaza1EFG) and Manhattan-136
    (tests/data/ManhattanPlaza136), n = 500 chains = ground truth + 0.03 N(0, 1) per coordinate, next to the
    nfisam_factor_graph_score + nfisam_factor_graph_log_density launches they sit between at the same shape: HIP events around
    the calls, tables uploaded, matrices in place; the two alternate over ROUNDS rounds of REPS calls, the median of a round's
    calls, then the median and range of the rounds' medians;
  * the small range problem (tests/golden, the recipe of the GPU tests): `posterior_mcmc` at its defaults for both kernels and
    with flow jumps -- acceptance rates, mean log p, mean log p - log q and the `posterior_ksd` V-statistic before and after.
No time and no improvement is asserted.  Prints one JSON object.   usage: sample_mcmc.py [out.json]"""
import json, os, random, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from test_sample_mcmc_cpu import accept, decision_cases, propose, rounding_bound, signed_wrap

REPS, ROUNDS = 20, 5
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


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


out = dict(what="the Metropolis proposal and accept step on one MI355X: scripts/sample_mcmc.py")

# ---- the device against the restatement ---------------------------------------------------------------------------------------------
vs = {}
for drift in (True, False):
    ulp_worst, b_worst, chains = 0.0, 0.0, 0
    for c in decision_cases(drift):
        Xt, Gx, Gy, lx, ly = dev(c["Xt"]), dev(c["Gx"]), dev(c["Gy"]), dev(c["lp_x"]), dev(c["lp_y"])
        Yt = nh.sample_propose_t(Xt, Gx, c["h"], c["wrap"], c["seed"], c["t"])
        Yd, Yr = Yt.cpu().numpy(), propose(c["Xt"], c["Gx"], c["h"], c["wrap"], c["seed"], c["t"])
        diff = Yd.astype(np.float64) - Yr
        if c["wrap"] is not None:
            w = c["wrap"].astype(bool)
            diff[w] = signed_wrap(diff[w])
        ulp_worst = max(ulp_worst, float(np.max(np.abs(diff) / np.spacing(np.maximum(np.abs(Yd), np.abs(Yr)).astype(np.float32)))))
        ref = accept(c["Xt"], Yd, c["Gx"], c["Gy"], c["lp_x"], c["lp_y"], c["h"], c["wrap"], c["seed"], c["t"])
        la, acc = nh.sample_accept_t(Xt, Yt, Gx, Gy, lx, ly, c["h"], c["wrap"], c["seed"], c["t"])
        B = rounding_bound(c["Xt"].shape[0], ref["abs_sum"])
        b_worst = max(b_worst, float(np.max(np.abs(la.cpu().numpy() - ref["log_alpha"]) / B)))
        assert np.array_equal(acc.cpu().numpy(), ref["accepted"])
        chains += c["Xt"].shape[1]
    vs["with_scores" if drift else "symmetric"] = dict(proposal_float32_ulp=ulp_worst, log_alpha_over_B=b_worst, chains=chains)
out["device_vs_numpy_restatement"] = vs
print("device against the restatement:", vs, flush=True)

# ---- the pair next to the evaluators it sits between ---------------------------------------------------------------------------------
timing = dict(reps=REPS, rounds=ROUNDS, n=500,
              stat="the two alternate over %d rounds; a round's figure is the median of %d calls after one warm-up call; "
                   "reported: the median and the range of the rounds" % (ROUNDS, REPS))
for name, folder in (("plaza1", "Plaza1EFG"), ("manhattan136", "ManhattanPlaza136")):
    nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", folder, "factor_graph.fg"), "fg",
                                              prior_cov_scale=0.1)
    col, D = {}, 0
    for v in nodes:
        col[v] = D
        D += v.dim
    circ = np.concatenate([[bool(c) for c in v.circular_dim_list] for v in nodes]).astype(np.uint8)
    t = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
    terms = nh.pack_factor_terms(factors, col)
    gather = nh.pack_score_gather(terms, D)
    terms_dev, = nh.upload(terms.view(np.uint8).reshape(-1), device=DEV, cached=True)
    n = 500
    rng = np.random.RandomState(0)
    St = dev((t + 0.03 * rng.randn(n, D)).astype(np.float32).T)
    h = np.where(circ != 0, 0.01, 0.02)
    tables = nh.mcmc_tables(DEV, h, circ)
    scratch = nh.sample_accept_scratch(D, n, DEV)
    Gx = nh.factor_graph_score_t(terms, St, DEV, gather=gather, terms_dev=terms_dev)
    lp = nh.factor_graph_log_density_t(terms, St, DEV, terms_dev=terms_dev, checked=True)
    Yt = nh.sample_propose_t(St, Gx, None, seed=1, t=0, checked=True, tables=tables)
    Gy = nh.factor_graph_score_t(terms, Yt, DEV, gather=gather, terms_dev=terms_dev)
    lp_y = nh.factor_graph_log_density_t(terms, Yt, DEV, terms_dev=terms_dev, checked=True)
    work, Gw, lw = St.clone(), Gx.clone(), lp.clone()
    torch.cuda.synchronize()

    def pair():
        nh.sample_propose_t(work, Gw, None, seed=1, t=0, Yt=Yt, checked=True, tables=tables)
        nh.sample_accept_t(work, Yt, Gw, Gy, lw, lp_y, None, seed=1, t=0, checked=True, tables=tables, scratch=scratch)

    def only_propose():
        nh.sample_propose_t(work, Gw, None, seed=1, t=0, Yt=Yt, checked=True, tables=tables)

    def only_accept():
        nh.sample_accept_t(work, Yt, Gw, Gy, lw, lp_y, None, seed=1, t=0, checked=True, tables=tables, scratch=scratch)

    def evaluators():
        nh.factor_graph_score_t(terms, Yt, DEV, gather=gather, terms_dev=terms_dev)
        nh.factor_graph_log_density_t(terms, Yt, DEV, terms_dev=terms_dev, checked=True)

    rounds = dict(pair=[], evaluators=[], propose=[], accept=[])
    for _ in range(ROUNDS):
        rounds["pair"].append(timed(pair))
        rounds["evaluators"].append(timed(evaluators))
        rounds["propose"].append(timed(only_propose))
        rounds["accept"].append(timed(only_accept))
    q = dict(x_rows=D, factors=int(terms.shape[0]), accept_slabs=(D + nh.MCMC_SLAB - 1) // nh.MCMC_SLAB,
             bytes_moved_by_the_pair=int(D * n * (4 + 8 + 4) + D * n * (4 + 4 + 8 + 8) + D * n * 2 * (4 + 8)))
    for k, v in rounds.items():
        q[k + "_us"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    q["pair_over_evaluators"] = q["pair_us"]["median"] / q["evaluators_us"]["median"]
    print("%s n = %d:" % (name, n), q, flush=True)
    timing[name] = q
    del St, Gx, Gy, Yt, work, Gw, scratch
    torch.cuda.empty_cache()
out["timing"] = timing

# ---- the small range problem: what the chains do to the trained posterior's draw -----------------------------------------------------------
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
for vs_, fs in steps:
    for v in vs_: solver.add_node(v)
    for f in fs: solver.add_factor(f)
    solver.update_physical_and_working_graphs()
    smp = solver.incremental_inference()
smp = {v: np.array(smp[v]) for v in solver.elimination_ordering}


def grade(s):
    d, k = solver.posterior_diagnostics(s), solver.posterior_ksd(s)
    return dict(vstat=k["vstat"], ustat=k["ustat"], mean_log_p=float(d["log_p"].mean()), mean_log_w=float(d["log_w"].mean()),
                ess=d["ess"])


small = dict(n=len(next(iter(smp.values()))), before=grade(smp))
for label, opts in (("mala", dict(kernel="mala")), ("rw", dict(kernel="rw")), ("mala_with_jumps", dict(independence_every=5)),
                    ("jumps_only", dict(independence_every=1, steps=20, warmup=0))):
    r = solver.posterior_mcmc(smp, seed=1, **opts)
    small[label] = dict(grade(r["samples"]), steps=r["steps"], warmup=r["warmup"], accept_rate=r["accept_rate"],
                        jump_accept_rate=r["jump_accept_rate"],
                        median_step_size=float(np.median([np.median(r["step_size"][v]) for v in r["step_size"]])))
    print("small range, %s:" % label, small[label], "before:", small["before"], flush=True)
out["small_range"] = small

print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
