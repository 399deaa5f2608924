"""The chain diagnostics (nfisam_chain_record, nfisam_chain_finish) on one MI355X:
  * how far the device lies from the float64 numpy restatement of tests/test_sample_chains_cpu.py at shapes of
    tests/test_sample_chains_gpu.py, as a fraction of the tests' derived bounds (for the record: the bounds are not measured);
  * device us of the record launch and of the finish on the row counts of Plaza1 (tests/data/Plaza1EFG) and Manhattan-136
    (tests/data/ManhattanPlaza136), n = 500 chains, 8 levels, T = 256, next to the propose + accept pair of the same run -- the
    yardstick: HIP events around the calls, tables uploaded, matrices in place; the sides alternate over ROUNDS rounds of REPS
    calls, the median of a round's calls, then the median and range of the rounds' medians.  The record launch is timed at
    t = 0 (one pending store), t = 1 (one level update), t = 127 (all seven levels update) and amortised over the 128 calls
    t = 0 ... 127 between one pair of events;
  * the small range problem (tests/golden, the recipe of the GPU tests): `posterior_mcmc` at its defaults with and without
    `diagnostics` (wall clock around the call, the device drained), and the R-hat and tau the default 200-step run reports.
No time is asserted.  Prints one JSON object.   usage: sample_chains.py [out.json]"""
import json, os, random, sys, tempfile, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from test_sample_chains_cpu import acc_bound, assert_within, finish, finish_bounds, history, max_levels, record_history

REPS, ROUNDS = 20, 5
DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
LEVELS, T_RUN = 8, 256


def timed(call, reps=REPS, per=1):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps + 1):
        ev0.record()
        call()
        ev1.record()
        ev1.synchronize()
        ts.append(ev0.elapsed_time(ev1) * 1e3 / per)
    return float(np.median(ts[1:]))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


out = dict(what="the chain diagnostics (record, finish) on one MI355X: scripts/sample_chains.py")

# ---- the device against the restatement ---------------------------------------------------------------------------------------------
worst_acc, worst_stat, cases = 0.0, 0.0, 0
for T in (4, 14, 64):
    for n in (1, 65, 130):
        for rows in (5, 67):
            hist, center, wrap = history(T, rows, n)
            levels = max_levels(T)
            Hd, tb = dev(hist), nh.chain_tables(DEV, center, wrap)
            state = nh.chain_state(rows, n, levels, DEV)
            for t in range(T):
                nh.chain_record_t(state, Hd[t], t, T, levels, tables=tb, checked=True)
            ref, ref_abs = record_history(hist, levels, center, wrap)
            err, B = np.abs(state.cpu().numpy() - ref), acc_bound(T, ref_abs)
            worst_acc = max(worst_acc, float(np.max(err[B > 0] / B[B > 0])))
            got = {k: v.cpu().numpy() for k, v in nh.chain_finish_t(state, rows, n, levels, T, tables=tb).items()}
            worst_stat = max(worst_stat, assert_within(got, finish(ref, T, levels, center, wrap),
                                                       finish_bounds(ref, ref_abs, T, levels, center), (T, n, rows), circular=wrap))
            cases += 1
out["device_vs_numpy_restatement"] = dict(cases=cases, accumulators_over_bound=worst_acc, statistics_over_bound=worst_stat)
print("device against the restatement:", out["device_vs_numpy_restatement"], flush=True)

# ---- the record launch and the finish next to the propose + accept pair ------------------------------------------------------------------
timing = dict(reps=REPS, rounds=ROUNDS, n=500, levels=LEVELS, T=T_RUN,
              stat="the sides alternate over %d rounds; a round's figure is the median of %d calls after one warm-up call; "
                   "reported: the median and the range of the rounds" % (ROUNDS, REPS))
for name, folder in (("plaza1", "Plaza1EFG"), ("manhattan136", "ManhattanPlaza136")):
    nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", folder, "factor_graph.fg"), "fg",
                                              prior_cov_scale=0.1)
    col, D = {}, 0
    for v in nodes:
        col[v] = D
        D += v.dim
    circ = np.concatenate([[bool(c) for c in v.circular_dim_list] for v in nodes]).astype(np.uint8)
    tr = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
    terms = nh.pack_factor_terms(factors, col)
    gather = nh.pack_score_gather(terms, D)
    terms_dev, = nh.upload(terms.view(np.uint8).reshape(-1), device=DEV, cached=True)
    n = 500
    rng = np.random.RandomState(0)
    St = dev((tr + 0.03 * rng.randn(n, D)).astype(np.float32).T)
    h = np.where(circ != 0, 0.01, 0.02)
    tables = nh.mcmc_tables(DEV, h, circ)
    scratch = nh.sample_accept_scratch(D, n, DEV)
    Gx = nh.factor_graph_score_t(terms, St, DEV, gather=gather, terms_dev=terms_dev)
    lp = nh.factor_graph_log_density_t(terms, St, DEV, terms_dev=terms_dev, checked=True)
    Yt = nh.sample_propose_t(St, Gx, None, seed=1, t=0, checked=True, tables=tables)
    Gy = nh.factor_graph_score_t(terms, Yt, DEV, gather=gather, terms_dev=terms_dev)
    lp_y = nh.factor_graph_log_density_t(terms, Yt, DEV, terms_dev=terms_dev, checked=True)
    work, Gw, lw = St.clone(), Gx.clone(), lp.clone()
    ctab = nh.chain_tables(DEV, tr, circ)
    state = nh.chain_state(D, n, LEVELS, DEV)
    torch.cuda.synchronize()

    def pair():
        nh.sample_propose_t(work, Gw, None, seed=1, t=0, Yt=Yt, checked=True, tables=tables)
        nh.sample_accept_t(work, Yt, Gw, Gy, lw, lp_y, None, seed=1, t=0, checked=True, tables=tables, scratch=scratch)

    def record_at(t):
        return lambda: nh.chain_record_t(state, work, t, T_RUN, LEVELS, checked=True, tables=ctab)

    def record_run():
        for t in range(128):
            nh.chain_record_t(state, work, t, T_RUN, LEVELS, checked=True, tables=ctab)

    def finish_call():
        nh.chain_finish_t(state, D, n, LEVELS, T_RUN, tables=ctab)

    rounds = dict(pair=[], record_t0=[], record_t1=[], record_t127=[], record_amortised=[], finish=[])
    for _ in range(ROUNDS):
        rounds["pair"].append(timed(pair))
        rounds["record_t0"].append(timed(record_at(0)))
        rounds["record_t1"].append(timed(record_at(1)))
        rounds["record_t127"].append(timed(record_at(127)))
        rounds["record_amortised"].append(timed(record_run, per=128))
        rounds["finish"].append(timed(finish_call))
    # bytes: the point (4) + A1, A2 read and written (32); level l is reached every 2^(l-1)-th step: half of those store P (8),
    # half read P and read and write R, Q (40): sum_l 24 / 2^(l-1) -> 48
    q = dict(x_rows=D, state_bytes=int(state.numel() * 8),
             bytes_moved_by_the_pair=int(D * n * (4 + 8 + 4) + D * n * (4 + 4 + 8 + 8) + D * n * 2 * (4 + 8)),
             bytes_moved_by_a_record_amortised=int(D * n * (4 + 32 + sum(24.0 / 2 ** (l - 1) for l in range(1, LEVELS)))),
             bytes_moved_by_the_finish=int(D * n * 8 * (4 + 2 + 2 * (LEVELS - 1))))
    for k, v in rounds.items():
        q[k + "_us"] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    q["record_amortised_over_pair"] = q["record_amortised_us"]["median"] / q["pair_us"]["median"]
    q["record_amortised_GBps"] = q["bytes_moved_by_a_record_amortised"] / q["record_amortised_us"]["median"] * 1e-3
    print("%s n = %d:" % (name, n), q, flush=True)
    timing[name] = q
    del St, Gx, Gy, Yt, work, Gw, scratch, state
    torch.cuda.empty_cache()
out["timing"] = timing

# ---- the small range problem: what the diagnostics say about the default run, and what they cost ------------------------------------------
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


def wall(diagnostics):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = solver.posterior_mcmc(smp, seed=1, diagnostics=diagnostics)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


wall(False), wall(True)                                                # (one warm-up call each)
ms = dict(off=[], on=[])
for _ in range(ROUNDS):
    ms["off"].append(wall(False)[0])
    t_on, res = wall(True)
    ms["on"].append(t_on)
small = dict(n=res["n"], steps=res["steps"], warmup=res["warmup"], recorded=res["recorded"], accept_rate=res["accept_rate"],
             rhat_max=res["rhat_max"], ess_min=res["ess_min"],
             posterior_mcmc_ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ms.items()},
             variables={str(v.name): {k: [float(x) for x in d[k]] for k in ("rhat", "tau", "ess", "resolved")}
                        for v, d in res["diagnostics"].items()})
small["diagnostics_over_plain"] = small["posterior_mcmc_ms"]["on"]["median"] / small["posterior_mcmc_ms"]["off"]["median"]
for name, d in small["variables"].items():
    print("small range, %s: R-hat %s tau %s ess %s resolved %s" % (name, d["rhat"], d["tau"], d["ess"], d["resolved"]), flush=True)
print("small range:", {k: v for k, v in small.items() if k != "variables"}, flush=True)
out["small_range"] = small

print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
