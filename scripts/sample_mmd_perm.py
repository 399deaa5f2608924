"""The MMD permutation test on the final Plaza1 tree: Plaza1 end to end (run_plaza1.py's defaults, as scripts/sample_mmd.py),
then the table `posterior_mmd` builds -- the joint xy block plus every variable's xy marginal -- for the posterior against a
second draw of itself, at n = m = 500 and 2000, with P = 999 relabellings of seed 0:
  * new: device us of nfisam_hip.mmd_perm_sums_t from HIP events around the call (matrices in place; the label upload and
    the binding's chunk loop are inside), all P permutations;
  * baseline: what there was before -- per permutation the pooled matrix index-gathered into its two relabelled sets and
    one `mmd_sums_t` call with the same table -- timed over the first P0 = 16 permutations and SCALED LINEARLY to P (every
    permutation costs the same: the same shapes, the same launches);
  * new and baseline alternate, ROUNDS rounds after one warm-up round; medians are reported, and their ratio;
  * ns per (block, ordered pooled pair, permutation) of the new kernel: new / (blocks * (m + n)^2 * P);
  * the float64 numpy oracle (direct differences, sub-matrix sums) on ONE xy block over the same P0 permutations, scaled
    the same way, for scale; and the largest |new - baseline| / T and |new - oracle| / T over what both computed;
  * wall s of NFiSAM.posterior_mmd_test(reference, samples), once.
Prints one JSON object.   usage: sample_mmd_perm.py [out.json]"""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT)
import nfisam_hip as nh
from slam.NFiSAM import NFiSAM, NFiSAMArgs
from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
from utils import Statistics as ST

ROUNDS, P, P0 = 5, 999, 16
DEV = "cuda:0"
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


def device_us(f):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    r = f()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) * 1e3, r


order = list(solver.elimination_ordering)
out = dict(dataset="Plaza1EFG", updates=len(steps), end_to_end_s=run_s, variables=len(order), blocks=len(order) + 1,
           joint_columns=2 * len(order), kernel="k_sigma2 = 1, xy columns", permutations=P, baseline_permutations=P0,
           rounds=ROUNDS, stat="new and baseline alternate; median of %d rounds after one warm-up round; the baseline and the "
           "oracle are timed over %d permutations and scaled by %d / %d" % (ROUNDS, P0, P, P0))
pcol, total_dim = solver._post_columns()
for n in (500, 2000):
    solver._args.posterior_sample_num = n
    smp = {v: np.array(a) for v, a in solver.sample_posterior().items()}
    ref = {v: np.array(a) for v, a in solver.sample_posterior().items()}
    X = np.zeros((n, total_dim), dtype=np.float32)
    Y = np.zeros((n, total_dim), dtype=np.float32)
    for v in order:
        X[:, pcol[v]:pcol[v] + v.dim] = smp[v]
        Y[:, pcol[v]:pcol[v] + v.dim] = ref[v]
    xy = [[pcol[v], pcol[v] + 1] for v in order]
    blocks = [[c for b in xy for c in b]] + xy
    cols = np.concatenate([np.asarray(b, dtype=np.int32) for b in blocks])
    table = nh.pack_mmd_blocks([len(b) for b in blocks], np.ones(len(blocks)))
    nh.check_mmd_blocks(table, cols, cols, total_dim, total_dim)
    Xt, Yt = torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV), torch.from_numpy(np.ascontiguousarray(Y.T)).to(DEV)
    Zt = torch.cat([Xt, Yt], dim=1).contiguous()
    L = ST.permutation_labels(n, n, P, seed=0)
    packed = nh.pack_perm_labels(L)
    nh.check_perm_labels(packed, n, n, P)
    first = [torch.from_numpy(np.flatnonzero(l)).to(DEV) for l in L[:P0]]
    second = [torch.from_numpy(np.flatnonzero(~l)).to(DEV) for l in L[:P0]]

    def new():
        return nh.mmd_perm_sums_t(Xt, Yt, table, cols, cols, packed, checked=True, n_perms=P)

    def baseline():
        return torch.stack([nh.mmd_sums_t(Zt[:, a].contiguous(), Zt[:, b].contiguous(), table, cols, cols, checked=True)
                            for a, b in zip(first, second)], dim=1)

    new_us, base_us = [], []
    for k in range(ROUNDS + 1):
        t_new, got = device_us(new)
        t_base, want = device_us(baseline)
        if k:
            new_us.append(t_new), base_us.append(t_base * P / P0)
    r = dict(new_us=float(np.median(new_us)), baseline_scaled_us=float(np.median(base_us)), new_us_rounds=new_us,
             baseline_scaled_us_rounds=base_us)
    r["speedup"] = r["baseline_scaled_us"] / r["new_us"]
    r["new_ns_per_block_pair_permutation"] = r["new_us"] * 1e3 / (len(blocks) * (2.0 * n) ** 2 * P)
    r["scratch_bytes_per_launch"] = 8 * int(nh.lib().nfisam_sample_mmd_perm_scratch_count(n, n, len(blocks), nh.MMD_PERM_CHUNK))
    got, want = got.cpu().numpy(), want.cpu().numpy()
    T = (want[:, 0, 0] + want[:, 0, 1] + 2.0 * want[:, 0, 2])[:, None, None]
    r["max_dev_from_baseline_over_T"] = float(np.max(np.abs(got[:, :P0] - want) / T))
    print("n = %d: new %.0f us, baseline (scaled) %.0f us, ratio %.1f" % (n, r["new_us"], r["baseline_scaled_us"], r["speedup"]),
          flush=True)
    # the numpy oracle on the first xy block, P0 permutations
    Z = np.concatenate([X[:, blocks[1]], Y[:, blocks[1]]], 0).astype(np.float64)
    a = time.perf_counter()
    K = np.empty((2 * n, 2 * n))
    for s in range(0, 2 * n, 256):
        diff = Z[s:s + 256, None, :] - Z[None, :, :]
        K[s:s + 256] = np.exp(-0.5 * np.einsum("ijk,ijk->ij", diff, diff))
    oracle = np.array([[K[np.ix_(l, l)].sum(), K[np.ix_(~l, ~l)].sum(), K[np.ix_(l, ~l)].sum()] for l in L[:P0]])
    r["numpy_oracle_one_block_scaled_us"] = (time.perf_counter() - a) * 1e6 * P / P0
    r["max_dev_from_oracle_over_T"] = float(np.max(np.abs(got[1, :P0] - oracle) / K.sum()))
    a = time.perf_counter()
    res = solver.posterior_mmd_test(ref, smp, permutations=P, seed=0)
    r["posterior_mmd_test_wall_s"] = time.perf_counter() - a
    r["joint_p_value"], r["rejected"] = res["p_value"]["joint"], len(res["rejected"])
    out["n%d" % n] = r

print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
