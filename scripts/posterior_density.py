"""Posterior log-density on the final Plaza1 tree: Plaza1 end to end (run_plaza1.py's defaults: K = 9, n = 2000, <= 2000
iterations, lr .01, window 50, tol .01, incremental_step = 5), then NFiSAM.posterior_log_pdf on the posterior samples at
n = 500 and n = 10 000: kernel us from HIP events around the launch (sample matrix and table already assembled; median of 20
calls, the first excluded), wall us of the whole call, and for comparison the per-clique composition through
nfisam_hip.forward(..., want_logprob=True) (two forwards per clique: the first D and the first n_obs + n_sep columns).
Prints one JSON object.   usage: posterior_density.py [out.json]"""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT)
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally

REPS = 20
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


def median_after_first(f):
    ts = [f() for _ in range(REPS + 1)]
    return float(np.median(ts[1:]))


def composition(t, S):
    """log q by one nfisam_hip.forward pair per clique (what a caller could do with the existing entries)."""
    total = torch.zeros(S.shape[0], dtype=torch.float32, device=S.device)
    for c in t["cliques"]:
        m = solver._clique_density_model[c]
        f0 = m.flows[0]
        e = m.__dict__["_post_entry"]
        n_obs, n_sep = e["obs"].size, int(np.frombuffer(e["row"], dtype=nh.POST_DTYPE)["n_sep"][0])
        idx = torch.as_tensor(e["cols"], dtype=torch.long, device=S.device)
        x = S[:, idx]
        if n_obs:
            x = torch.cat([torch.as_tensor(e["obs"], device=S.device).expand(S.shape[0], -1), x], 1)
        xn = m.normalize_samples(x.clone(), init_dim=0).contiguous()
        Ds = n_obs + n_sep
        _, _, lp = nh.forward(xn, m.kernel_params(), f0.K, f0.hidden_dim, f0.B, len(m.flows), want_z=False,
                              want_logdet=False, want_logprob=True, model_D=f0.dim)
        if Ds:
            _, _, lps = nh.forward(xn[:, :Ds].contiguous(), m.kernel_params(), f0.K, f0.hidden_dim, f0.B, len(m.flows),
                                   want_z=False, want_logdet=False, want_logprob=True, model_D=f0.dim)
            lp = lp - lps
        std = torch.as_tensor(m.samples_std, dtype=torch.float32).to(S.device)
        total = total + lp - torch.log(std[Ds:x.shape[1]]).sum()
    return total


out = dict(dataset="Plaza1EFG", updates=len(steps), end_to_end_s=run_s, variables=len(solver.physical_vars),
           reps=REPS, stat="median of %d calls, the first excluded" % REPS)
t = solver._posterior_table()
K, H, B, L = t["cfg"]
out["cliques"] = len(t["cliques"])
out["frontal_columns"] = int(t["table"]["n_frontal"].sum())
out["max_D"] = int(t["max_D"])
for n in (500, 10000):
    solver._args.posterior_sample_num = n
    smp = solver.sample_posterior()
    lq = solver.posterior_log_pdf(smp)
    r = dict(finite=bool(np.all(np.isfinite(lq))), mean_log_q=float(lq.mean()))

    def wall():
        a = time.perf_counter()
        solver.posterior_log_pdf(smp)
        return (time.perf_counter() - a) * 1e6
    r["wall_us"] = median_after_first(wall)
    S = torch.zeros(n, t["total_dim"], dtype=torch.float32, device=t["device"])
    for v in solver.elimination_ordering:
        S[:, t["pcol"][v]:t["pcol"][v] + v.dim] = torch.from_numpy(np.ascontiguousarray(smp[v], dtype=np.float32))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    St = S.t().contiguous()
    tbl, cols_t, obs_t = nh.upload(t["table"].view(np.uint8).reshape(-1), t["cols"], t["obs"], device=t["device"], cached=True)
    log_q = torch.empty(n, dtype=torch.float32, device=t["device"])
    per = torch.empty(len(t["cliques"]), n, dtype=torch.float32, device=t["device"])
    import ctypes as C

    def kernel():
        ev0.record()
        nh._check(nh.lib().nfisam_nsf_posterior_log_density(C.c_void_p(tbl.data_ptr()), len(t["cliques"]), nh._ptr(cols_t),
                                                             nh._ptr(obs_t), int(t["max_D"]), K, H, C.c_float(B), L, n,
                                                             nh._ptr(St), nh._ptr(log_q), nh._ptr(per), None, nh._stream()),
                  "nfisam_nsf_posterior_log_density")
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3
    r["kernel_us"] = median_after_first(kernel)
    r["kernel_equals_solver_call"] = bool(np.array_equal(log_q.cpu().numpy(), lq))

    def comp():
        torch.cuda.synchronize()
        a = time.perf_counter()
        q = composition(t, S)
        torch.cuda.synchronize()
        return (time.perf_counter() - a) * 1e6
    c0 = composition(t, S).cpu().numpy()
    r["composition_wall_us"] = median_after_first(comp)
    r["composition_max_abs_diff"] = float(np.abs(c0 - lq).max())
    r["speedup_vs_composition_kernel"] = r["composition_wall_us"] / r["kernel_us"]
    r["speedup_vs_composition_wall"] = r["composition_wall_us"] / r["wall_us"]
    out["n%d" % n] = r
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
