"""k nearest neighbours and ball counts on a Plaza1-sized table: one block per variable of a 780-variable graph (every fifth a
2-column landmark, the others 3-column poses with a wrapped heading), n = 2000 posterior points, k = 4, max norm --
synthetic points: the kernels' work depends on the table's shape and on n alone.
  * device us of the C entries between HIP events (20 replays after 5 warm-ups: median, min, max; matrix in place, tables
    uploaded per call, outputs allocated): nfisam_sample_knn with its log_sum launch, nfisam_sample_ball_count with the
    k-th distances as radii; both norms,
  * wall us of utils.Statistics.knn_entropy_t on that table (moments for the scales, the search, the host formula) and of
    knn_mutual_information_t on the 779 consecutive pairs,
  * for scale, on the host: scipy.spatial.cKDTree (one tree and one query per block, p = inf) and a numpy brute force
    (the oracle of tests/test_sample_knn_cpu.py) over the same blocks, the latter on the first 20 and scaled up,
  * that the device's k-th distances are the cKDTree's on every block (up to the rounding of the tree's scaled points),
  * with --tests: the largest error / bound ratio over the GPU tests' cases, and the largest ulp error of the device's log
    over their distances (the LOG_ULP the tests' log_sum bound is built from),
  * the compiler's resource figures of the unit (recorded below from its report).
No time is asserted anywhere; the parent commit has no counterpart.  Prints one JSON object and writes it to out.json.
usage: sample_knn.py [--tests] [out.json (default profiles/knn.json)]"""
import contextlib, io, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nf-isam_amd")); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import nfisam_hip as nh
from utils import Statistics as ST

REPS, WARM = 20, 5
DEV = "cuda:0"
# hipcc -O3 -ffp-contract=fast --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on sample_knn.hip
RESOURCES = {"knn_kernel<4, max>": dict(vgprs=137, scratch_bytes_per_lane=0, lds_bytes=24896, waves_per_simd=3),
             "knn_kernel<16, max>": dict(vgprs=173, scratch_bytes_per_lane=0, lds_bytes=61760, waves_per_simd=2),
             "knn_kernel<4, l2>": dict(vgprs=146, scratch_bytes_per_lane=0, lds_bytes=24896, waves_per_simd=3),
             "knn_kernel<16, l2>": dict(vgprs=182, scratch_bytes_per_lane=0, lds_bytes=61760, waves_per_simd=2),
             "ball_kernel<max>": dict(vgprs=122, scratch_bytes_per_lane=0, lds_bytes=13632, waves_per_simd=4),
             "ball_kernel<l2>": dict(vgprs=136, scratch_bytes_per_lane=0, lds_bytes=13632, waves_per_simd=3),
             "knn_log_sum_kernel": dict(vgprs=40, scratch_bytes_per_lane=0, lds_bytes=48, waves_per_simd=8)}
flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "knn.json")


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


V, N, K = 780, 2000, 4
rng = np.random.RandomState(0)
dims = np.where(np.arange(V) % 5 == 4, 2, 3)
width = int(dims.sum())
start = np.cumsum(dims) - dims
X = (rng.normal(size=(N, width)) * rng.uniform(0.05, 3.0, width) + rng.uniform(-100, 100, width)).astype(np.float32)
circ = np.zeros(width, dtype=bool)
circ[start[dims == 3] + 2] = True
X[:, circ] = ((rng.normal(size=(N, int(circ.sum()))) * 0.3 + rng.uniform(-np.pi, np.pi, int(circ.sum())) + np.pi) % (2 * np.pi) - np.pi).astype(np.float32)
blocks = [np.arange(s, s + d) for s, d in zip(start, dims)]
St = nh._columns(X, DEV)
cols = np.arange(width, dtype=np.int32)
table = nh.pack_knn_blocks(dims)
wrap = circ.astype(np.uint8)
ent = ST.knn_entropy_t(St, blocks, K, circ)
scale = ent["scale"]

out = dict(table=dict(blocks=V, columns=width, n=N, k=K, poses=int((dims == 3).sum()), landmarks=int((dims == 2).sum())), reps=REPS,
           warmups=WARM, stat="median / min / max of the replays after the warm-ups, us",
           pair_distances=float(V) * N * N)
for norm in ("max", "l2"):
    buf = nh.sample_knn_t(St, None, table, cols, cols, K, norm, scale, wrap, True, checked=True)
    r = {}
    r["knn_entry_device_us"], r["knn_entry_wall_us"] = timed(
        lambda: nh.sample_knn_t(St, None, table, cols, cols, K, norm, scale, wrap, True, checked=True, out=buf))
    eps = buf["dist"][:, K - 1, :].contiguous()
    rows = table.copy()
    rows["radius_row"] = np.arange(V)
    cnt = nh.sample_ball_count_t(St, None, rows, cols, cols, eps, norm, scale, wrap, True, checked=True)
    r["ball_count_entry_device_us"], r["ball_count_entry_wall_us"] = timed(
        lambda: nh.sample_ball_count_t(St, None, rows, cols, cols, eps, norm, scale, wrap, True, checked=True, out=cnt))
    r["pair_distances_per_us_knn"] = out["pair_distances"] / r["knn_entry_device_us"]["median"]
    # strict: the k-th neighbour is outside its own radius; fewer than k - 1 inside means a tie at the k-th distance
    r["share_of_counts_equal_to_k_minus_1"] = float((cnt == K - 1).double().mean().item())
    out[norm] = r
    print("%s: knn %.0f us, ball count %.0f us on the device" % (norm, r["knn_entry_device_us"]["median"],
                                                                  r["ball_count_entry_device_us"]["median"]), flush=True)
REPS, WARM = 5, 2
_, out["knn_entropy_t_wall_us"] = timed(lambda: ST.knn_entropy_t(St, blocks, K, circ))
pairs = [(blocks[b], blocks[b + 1]) for b in range(V - 1)]
_, out["knn_mutual_information_t_wall_us_779_pairs"] = timed(lambda: ST.knn_mutual_information_t(St, pairs, K, circ))

# the host, for scale
from scipy.spatial import cKDTree
from test_sample_knn_cpu import oracle_dist, oracle_knn, wrap_pi
raw = nh.sample_knn_t(St, None, table, cols, cols, K, "max", scale, None, True, checked=True)     # (no wrap: what a k-d tree sees)
dev_eps = raw["dist"][:, K - 1, :].cpu().numpy()
t0 = time.perf_counter()
same = True
for b, c in enumerate(blocks):
    Z = X[:, c].astype(np.float64) * scale[c]
    dist, _ = cKDTree(Z).query(Z, k=K + 1, p=np.inf)
    # the tree scales the points, not the differences: each scaled coordinate carries a rounding of its own magnitude
    same = same and bool(np.all(np.abs(dist[:, K] - dev_eps[b]) <= 4 * 2.0 ** -53 * np.abs(Z).max()))
out["host_ckdtree_wall_us"] = (time.perf_counter() - t0) * 1e6
out["device_k_th_distance_equals_ckdtree_up_to_the_rounding_of_its_scaled_points"] = same
t0 = time.perf_counter()
for c in blocks[:20]:
    oracle_knn(oracle_dist(X, X, c, c, scale[c], wrap[c]), K, True)
out["host_numpy_brute_force_wall_us_scaled_from_20_blocks"] = (time.perf_counter() - t0) * 1e6 * V / 20
print("host: cKDTree %.2f s, numpy brute force about %.1f s" % (out["host_ckdtree_wall_us"] / 1e6,
                                                                out["host_numpy_brute_force_wall_us_scaled_from_20_blocks"] / 1e6), flush=True)

if "--tests" in flags:                                              # error / bound over the GPU tests' own cases
    import test_sample_knn_gpu as G
    recorded, G.LOG_ULP = G.LOG_ULP, float("inf")                   # (measured here, not asserted)
    with contextlib.redirect_stdout(io.StringIO()):                 # (the tests print every figure)
        for norm in ("max", "l2"):
            for k in (1, 4, 16):
                for m, n, ex in G.SHAPES:
                    G.test_neighbours_match_the_oracle(m, n, ex, k, norm)
            G.test_duplicates_ties_and_a_nan_coordinate(norm)
    log_ulp = G._worst.pop("device_log_ulp")
    G.LOG_ULP = recorded
    G._worst.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        for norm in ("max", "l2"):
            for k in (1, 4, 16):
                for m, n, ex in G.SHAPES:
                    G.test_neighbours_match_the_oracle(m, n, ex, k, norm)
            G.test_duplicates_ties_and_a_nan_coordinate(norm)
            G.test_statistics_knn_entropy(norm)
            G.test_statistics_knn_divergence(norm)
    G._worst.pop("device_log_ulp", None)
    out["largest_ratio"] = dict(error_over_bound_in_the_gpu_tests=dict(G._worst), device_log_largest_error_ulp=log_ulp,
                                log_ulp_the_tests_take=G.LOG_ULP,
                                rule="the bounds of tests/test_sample_knn_gpu.py (its docstring states them)")
out["resources"] = RESOURCES
print(json.dumps(out))
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
