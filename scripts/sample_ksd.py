"""Kernel Stein discrepancy at the shapes of the bundled graphs: Manhattan-136 (tests/data/ManhattanPlaza136) and Plaza1-ADA
(tests/data/Plaza1ADA0.4EFG), n = 500 points = ground truth + 0.03 N(0, 1) per coordinate, p = 1 / (D var), headings wrapped:
  * parity: the device score against the host `grad_x_log_pdf` sum, the device Stein sums against a float64 numpy
    restatement (that of tests/test_sample_ksd_cpu.py `stein_matrix`, 25 rows of i at a time), largest |device - numpy| / (|numpy| + 1),
  * device us of nfisam_factor_graph_score and of nfisam_sample_ksd from HIP events around the calls (tables uploaded,
    matrices in place; median of 20 calls after one warm-up call), wall us of the numpy restatement (once),
  * the same kernel at n = 1000 and 2000 (the points cycled with fresh noise): a tile of 64 x 64 pairs is one block, so
    n = 500 launches 64 blocks on a device with 256 compute units; us per (pair, column) against n shows what that leaves idle.
No time is asserted.  Prints one JSON object.   usage: sample_ksd.py [out.json]"""
import ctypes as C
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from slam.RunBatch import graph_file_parser
from test_factor_score_cpu import deviation, host_joint_score

REPS = 20
DEV = "cuda:0"
GRAPHS = {"manhattan136": "ManhattanPlaza136", "plaza1ada": "Plaza1ADA0.4EFG"}


def median_after_first(f, reps=REPS):
    ts = [f() for _ in range(reps + 1)]
    return float(np.median(ts[1:]))


def timed(call):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        ev0.record()
        call()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3
    return median_after_first(once)


out = dict(reps=REPS, stat="median of %d calls after one warm-up call; numpy once" % REPS)
for key, folder in GRAPHS.items():
    nodes, truth, factors = graph_file_parser(os.path.join(ROOT, "tests", "data", folder, "factor_graph.fg"), "fg",
                                              prior_cov_scale=0.1)
    col, D = {}, 0
    for v in nodes:
        col[v] = D
        D += v.dim
    circ = np.concatenate([[bool(c) for c in v.circular_dim_list] for v in nodes])
    t = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
    terms = nh.pack_factor_terms(factors, col)
    gather = nh.pack_score_gather(terms, D)
    rng = np.random.RandomState(0)
    r = dict(D=D, factors=len(factors), slots=gather["n_slots"], longest_row=int(np.diff(gather["row_off"]).max()))
    for n in (500, 1000, 2000):
        x = (t + 0.03 * rng.randn(n, D)).astype(np.float32)
        St = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
        p = 1.0 / (D * x.astype(np.float64).var(0))
        dev = nh._upload_named(DEV, terms=nh._table_bytes(terms), slot_off=gather["slot_off"], row_off=gather["row_off"],
                               row_slot=gather["row_slot"], p=p, wrap=circ.astype(np.uint8))
        Gt = torch.empty(D, n, dtype=torch.float64, device=DEV)
        vals = torch.empty(gather["n_slots"], n, dtype=torch.float64, device=DEV)
        scratch = torch.empty(int(nh.lib().nfisam_sample_ksd_scratch_count(n)), dtype=torch.float64, device=DEV)
        row, diag = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()

        def score():
            nh._check(nh.lib().nfisam_factor_graph_score(nh._ptr(dev["terms"]), len(factors), nh._ptr(St), D, n,
                                                         nh._ptr(dev["slot_off"]), gather["n_slots"], nh._ptr(dev["row_off"]),
                                                         nh._ptr(dev["row_slot"]), nh._ptr(Gt), nh._ptr(vals), nh._stream()),
                      "nfisam_factor_graph_score")

        def ksd():
            nh._check(nh.lib().nfisam_sample_ksd(nh._ptr(St), nh._ptr(Gt), D, n, nh._ptr(dev["p"]), nh._ptr(dev["wrap"]),
                                                 nh._ptr(row), nh._ptr(diag), None, nh._ptr(scratch), nh._stream()),
                      "nfisam_sample_ksd")
        q = dict(score_us=timed(score), ksd_us=timed(ksd), blocks=((n + 63) // 64) ** 2)
        q["ksd_ps_per_pair_column"] = q["ksd_us"] * 1e6 / (n * n * D)
        if n == 500:
            G = Gt.t().cpu().numpy()
            a = time.perf_counter()
            host = host_joint_score(factors, col, x)
            q["host_score_wall_us"] = (time.perf_counter() - a) * 1e6
            q["score_dev_vs_host"] = deviation(G, host)
            out_rows = row.cpu().numpy()
            # the restatement, 25 rows of i at a time (the full broadcast would be n x n x D doubles)
            x64 = x.astype(np.float64)
            worst, a = 0.0, time.perf_counter()
            for i0 in range(0, n, 25):
                d = x64[i0:i0 + 25, None, :] - x64[None, :, :]
                m = (np.abs(d) + np.pi) % (2.0 * np.pi) - np.pi
                d = np.where(circ[None, None, :], np.sign(d) * m, d)
                pd = p * d
                k = np.exp(-0.5 * (pd * d).sum(-1))
                H = k * (G[i0:i0 + 25] @ G.T + ((G[i0:i0 + 25, None, :] - G[None, :, :]) * pd).sum(-1) - (pd * pd).sum(-1) + p.sum())
                worst = max(worst, deviation(out_rows[i0:i0 + 25], H.sum(1)))
            q["numpy_wall_us"] = (time.perf_counter() - a) * 1e6
            q["ksd_dev_vs_numpy"] = worst
            q["speedup_vs_numpy_kernel"] = q["numpy_wall_us"] / q["ksd_us"]
            rs, ds = out_rows.sum(), diag.cpu().numpy().sum()
            q["vstat"], q["ustat"] = rs / (n * n), (rs - ds) / (n * (n - 1))
        print(key, "n = %d:" % n, q, flush=True)
        r["n%d" % n] = q
    out[key] = r
print(json.dumps(out))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
