"""utils.Statistics — maximum mean discrepancy used as the posterior parity metric
(reference: src/utils/Statistics.py:13-84; the biased estimator `MMDb` with an RBF kernel of
bandwidth sigma is what the reference's evaluation scripts report,
example/slam/small_range_gaussian_problem/icra_paper/mmd_rmse_time_da_plot_grid.py:167,245), and the summaries of a
sample set (reference: src/utils/Statistics.py:142-214): means with circular means for headings, covariances, resultant
lengths and quantiles on the device, the modes of a multi-modal sample set (mean-shift on the device), `rmse`,
`translation_distance` and `geodesic_distance` on the host; and the Gaussian kernel Stein discrepancy of a sample set
against the density's own score (reference: src/utils/Statistics.py:193-245), its pairwise sums on the device; and -- not
in the reference -- differential entropy, mutual information and a two-sample KL divergence by k nearest neighbours, the
neighbour search on the device, and the sliced Wasserstein distance between two sample sets, every projection, sort and
quantile integral on the device."""
import functools
import math

import numpy as np


def _rbf_gram(x: np.ndarray, y: np.ndarray, sigma: float) -> np.ndarray:
    d2 = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T
    return np.exp(-np.maximum(d2, 0.0) / (2.0 * sigma ** 2))


def MMDb(x: np.ndarray, y: np.ndarray, sigma: float = None) -> float:
    """Biased MMD estimate sqrt(mean k(x,x) + mean k(y,y) - 2 mean k(x,y)); sigma defaults to sqrt(dim)."""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    if sigma is None:
        sigma = np.sqrt(x.shape[1])
    v = _rbf_gram(x, x, sigma).mean() + _rbf_gram(y, y, sigma).mean() - 2.0 * _rbf_gram(x, y, sigma).mean()
    return float(np.sqrt(max(v, 0.0)))


def MMDu2(x: np.ndarray, y: np.ndarray, sigma: float = None) -> float:
    """Unbiased estimate of MMD^2 (may be negative)."""
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    if sigma is None:
        sigma = np.sqrt(x.shape[1])
    m, n = x.shape[0], y.shape[0]
    kxx, kyy = _rbf_gram(x, x, sigma), _rbf_gram(y, y, sigma)
    return float((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (n * (n - 1)) -
                 2.0 * _rbf_gram(x, y, sigma).mean())


def mmd(samples1: np.ndarray, samples2: np.ndarray, k_sigma2: float = 1.0) -> np.ndarray:
    """The reference's `mmd` (src/utils/Statistics.py:13-45; what icra_paper/compute_mmd.py writes to `run1/mmd`):
    sqrt(E1 + E2 - 2 E3) with the Gaussian kernel k(d) = N(d; 0, k_sigma2 I) / N(0; 0, k_sigma2 I) = exp(-|d|^2 / (2 k_sigma2)),
    E1 / E2 without the diagonal (means over i != j), E3 over all pairs.  Returns a one-element array like the
    reference (callers index `[0]`); NaN when the unbiased combination is negative, as there.  Vectorised."""
    x, y = np.atleast_2d(samples1).astype(np.float64), np.atleast_2d(samples2).astype(np.float64)
    m, n = x.shape[0], y.shape[0]
    s = np.sqrt(k_sigma2)
    kxx, kyy = _rbf_gram(x, x, s), _rbf_gram(y, y, s)
    e1 = (kxx.sum() - np.trace(kxx)) / (m * (m - 1))
    e2 = (kyy.sum() - np.trace(kyy)) / (n * (n - 1))
    e3 = _rbf_gram(x, y, s).mean()
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.array([e1 + e2 - 2.0 * e3]))


# ---- many column blocks at once, on the device (nfisam_sample_mmd) ------------------------------------------------------------
ESTIMATORS = ("MMDb", "MMDu2", "mmd")


def mmd_from_sums(sums: np.ndarray, m: int, n: int, estimator: str = "MMDb") -> np.ndarray:
    """The estimators above from the kernel sums {Sxx, Syy, Sxy} over ALL ordered pairs (diagonal included: it contributes
    exactly m and n), sums [n_blocks, 3] -> [n_blocks]:
    "MMDb" sqrt(max(Sxx / m^2 + Syy / n^2 - 2 Sxy / mn, 0)); "MMDu2" the same with the diagonals removed and means over
    i != j (may be negative); "mmd" the reference's: the sqrt of the MMDu2 value, NaN when that is negative."""
    if estimator not in ESTIMATORS:
        raise ValueError("estimator must be one of %s, got %r" % (ESTIMATORS, estimator))
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    m, n = int(m), int(n)
    if m < 1 or n < 1:
        raise ValueError("both sample sets need at least one point")
    sxx, syy, sxy = sums[:, 0], sums[:, 1], sums[:, 2]
    if estimator == "MMDb":
        return np.sqrt(np.maximum(sxx / (m * m) + syy / (n * n) - 2.0 * sxy / (m * n), 0.0))
    if m < 2 or n < 2:
        raise ValueError("%s needs at least two points in each set (m = %d, n = %d)" % (estimator, m, n))
    u2 = (sxx - m) / (m * (m - 1)) + (syy - n) / (n * (n - 1)) - 2.0 * sxy / (m * n)
    if estimator == "MMDu2":
        return u2
    with np.errstate(invalid="ignore"):
        return np.sqrt(u2)


def mmd_bandwidths(dims, estimator: str, sigma=None) -> np.ndarray:
    """THE rule for the kernel bandwidths of blocks of `dims` entries -> float64, one per block: sigma None gives 1 for "mmd"
    (the reference's k_sigma2 = 1) and sqrt(d) for "MMDb" / "MMDu2"; one value (0-d) is every block's; a list is taken as it
    is, flattened -- whether it has one value per block, and positive ones, the caller checks in its own words."""
    dims = np.asarray(dims)
    if sigma is None:
        return np.ones(dims.size) if estimator == "mmd" else np.sqrt(dims.astype(np.float64))
    sig = np.asarray(sigma, dtype=np.float64)
    return np.broadcast_to(sig, (dims.size,)) if sig.ndim == 0 else sig.reshape(-1)


def _block_pairs(blocks):
    """blocks -> [(xcols, ycols)]: a block is a list of column indices (both sets) or an (xcols, ycols) pair of lists."""
    out = []
    for k, b in enumerate(blocks):
        if isinstance(b, (tuple, list)) and len(b) == 2 and all(np.ndim(c) == 1 for c in b):
            xc, yc = (np.asarray(c, dtype=np.int64) for c in b)
        else:
            xc = yc = np.asarray(b, dtype=np.int64)
        if xc.ndim != 1 or xc.size < 1 or xc.shape != yc.shape:
            raise ValueError("block %d: a block is a non-empty list of columns, or two such lists of equal length" % k)
        out.append((xc, yc))
    if not out:
        raise ValueError("no blocks")
    return out


def mmd_blocks(x, y, blocks, estimator: str = "MMDb", sigma=None, scale=None, circular=None, device=None) -> np.ndarray:
    """The MMD between the sample sets x [m, x_cols] and y [n, y_cols] (numpy or torch) restricted to each of `blocks`, all
    blocks in ONE device launch (nfisam_hip.mmd_sums: float32 points, float64 arithmetic by direct differences) -> [n_blocks].

    blocks: list of column-index lists that apply to both sets, or of (xcols, ycols) pairs when the sets order their
    columns differently.  estimator: see `mmd_from_sums`.  sigma: None (sqrt(d) per block for "MMDb" / "MMDu2" like the
    functions above, k_sigma2 = 1 for "mmd"), one bandwidth, or one per block.  scale [x_cols]: factor on the differences of a
    column of x (and its partner in y), e.g. 1 / std.  circular [x_cols]: columns that are angles, compared by differences
    wrapped into [-pi, pi).  "MMDu2" and "mmd" need m, n >= 2 (ValueError).  There is no CPU path."""
    import nfisam_hip as _nh
    table, xcols, ycols, sc, wr, m, n = _mmd_block_tables(x, y, blocks, estimator, sigma, scale, circular)
    sums = _nh.mmd_sums(x, y, table, xcols, ycols, scale=sc, wrap=wr, device=device)
    return mmd_from_sums(sums.cpu().numpy(), m, n, estimator)


def _mmd_block_tables(x, y, blocks, estimator, sigma, scale, circular):
    """The argument checks and defaults of `mmd_blocks` (and of `mmd_permutation_test`, which shares them)
    -> (block table, xcols, ycols, scale per entry or None, wrap per entry or None, m, n).  No device."""
    import nfisam_hip as _nh
    if estimator not in ESTIMATORS:
        raise ValueError("estimator must be one of %s, got %r" % (ESTIMATORS, estimator))
    if np.ndim(x) != 2 or np.ndim(y) != 2:
        raise ValueError("x and y must be [points, columns]")
    m, n = int(x.shape[0]), int(y.shape[0])
    if m < 1 or n < 1 or (estimator != "MMDb" and (m < 2 or n < 2)):
        raise ValueError("%s needs at least %d points in each set (m = %d, n = %d)"
                         % (estimator, 1 if estimator == "MMDb" else 2, m, n))
    pairs = _block_pairs(blocks)
    dims = np.array([p[0].size for p in pairs])
    sig = mmd_bandwidths(dims, estimator, sigma)
    if sig.size != len(pairs):
        raise ValueError("sigma: one value, or one per block (%d), got %d" % (len(pairs), sig.size))
    xcols = np.concatenate([p[0] for p in pairs])
    ycols = np.concatenate([p[1] for p in pairs])
    if xcols.min() < 0 or xcols.max() >= x.shape[1] or ycols.min() < 0 or ycols.max() >= y.shape[1]:
        raise ValueError("a block names a column outside its sample set")
    sc = wr = None
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64).reshape(-1)
        if scale.size != x.shape[1]:
            raise ValueError("scale: one value per column of x (%d), got %d" % (x.shape[1], scale.size))
        sc = scale[xcols]
    if circular is not None:
        circular = np.asarray(circular, dtype=bool).reshape(-1)
        if circular.size != x.shape[1]:
            raise ValueError("circular: one flag per column of x (%d), got %d" % (x.shape[1], circular.size))
        wr = circular[xcols].astype(np.uint8)
    return _nh.pack_mmd_blocks(dims, sig), xcols, ycols, sc, wr, m, n


# ---- what an MMD value is worth: the permutation test (nfisam_sample_mmd_perm) -------------------------------------------------
def permutation_labels(m: int, n: int, permutations: int, seed) -> np.ndarray:
    """The relabellings of a permutation test of m + n pooled points -> bool [permutations, m + n], row p True where a
    point counts as the first set.  A CONTRACT, so that a seed names the same test everywhere:
    rng = np.random.Generator(np.random.PCG64(seed)), and row p has its m ones at rng.permutation(m + n)[:m], the rows drawn
    in order p = 0, 1, ..."""
    m, n, permutations = int(m), int(n), int(permutations)
    if m < 1 or n < 1:
        raise ValueError("both sample sets need at least one point")
    if permutations < 1:
        raise ValueError("permutations must be >= 1, got %d" % permutations)
    rng = np.random.Generator(np.random.PCG64(seed))
    L = np.zeros((permutations, m + n), dtype=np.bool_)
    for p in range(permutations):
        L[p, rng.permutation(m + n)[:m]] = True
    return L


def _null_shapes(statistic, null):
    """-> (statistic [nb], null [nb, P >= 1]) as float64 arrays."""
    statistic, null = np.asarray(statistic, dtype=np.float64).reshape(-1), np.asarray(null, dtype=np.float64)
    null = null.reshape(statistic.size, -1)
    if null.shape[1] < 1:
        raise ValueError("the null distribution needs at least one value per block")
    return statistic, null


def permutation_p_value(statistic, null) -> np.ndarray:
    """(1 + #{null >= statistic}) / (1 + P) per block: statistic [nb], null [nb, P] -> [nb].  Exact under exchangeability,
    never 0.  For the estimator "mmd" (a square root, NaN where MMDu2 is negative) pass the MMDu2 values of both: the
    square root is monotone, so it is the same test, and no NaN enters a comparison (`mmd_permutation_test` does so)."""
    statistic, null = _null_shapes(statistic, null)
    if np.isnan(statistic).any() or np.isnan(null).any():
        raise ValueError("NaN in the statistic or its null distribution (compare \"mmd\" on its MMDu2 values)")
    return (1.0 + (null >= statistic[:, None]).sum(axis=1)) / (1.0 + null.shape[1])


def permutation_threshold(statistic, null, alpha: float = 0.05) -> np.ndarray:
    """The (1 - alpha) quantile of the null distribution with the observed value included, per block: the smallest of the
    P + 1 values that at most alpha (P + 1) of them exceed -- a statistic above it has p_value <= alpha."""
    statistic, null = _null_shapes(statistic, null)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1), got %r" % (alpha,))
    pooled = np.sort(np.concatenate([null, statistic[:, None]], axis=1), axis=1)
    k = int(np.ceil((1.0 - alpha) * pooled.shape[1] - 1e-9)) - 1         # (1 - 0.05) * 1000 must count as 950, not 950.0000000000001
    return pooled[:, min(max(k, 0), pooled.shape[1] - 1)]


def holm_adjust(p) -> np.ndarray:
    """Holm's step-down adjusted p-values: with p sorted ascending, p_(k) -> max_{j <= k} min(1, (K - j + 1) p_(j)); a
    hypothesis is rejected at family-wise level alpha when its adjusted value is <= alpha.  Same shape as `p`."""
    p = np.asarray(p, dtype=np.float64)
    flat = p.reshape(-1)
    if flat.size == 0:
        return p.copy()
    if np.isnan(flat).any() or flat.min() < 0.0 or flat.max() > 1.0:
        raise ValueError("p-values must lie in [0, 1]")
    order = np.argsort(flat, kind="stable")
    adj = np.minimum(1.0, (flat.size - np.arange(flat.size)) * flat[order])
    out = np.empty_like(flat)
    out[order] = np.maximum.accumulate(adj)
    return out.reshape(p.shape)


def permutation_test_from_sums(obs_sums, null_sums, m: int, n: int, estimator: str = "MMDb", alpha: float = 0.05) -> dict:
    """The test's numbers from the kernel sums: obs_sums [nb, 3] (`mmd_sums`), null_sums [nb, P, 3] (`mmd_perm_sums`)
    -> dict(statistic [nb], null [nb, P], p_value, threshold, p_holm).  "mmd" is compared on its MMDu2 values, reported as
    the square roots (NaN where MMDu2 is negative; its threshold is NaN then too)."""
    obs_sums, null_sums = np.asarray(obs_sums, dtype=np.float64), np.asarray(null_sums, dtype=np.float64)
    nb, P = null_sums.shape[0], null_sums.shape[1]
    stat = mmd_from_sums(obs_sums, m, n, estimator)
    null = mmd_from_sums(null_sums.reshape(-1, 3), m, n, estimator).reshape(nb, P)
    if estimator == "mmd":
        cmp_stat = mmd_from_sums(obs_sums, m, n, "MMDu2")
        cmp_null = mmd_from_sums(null_sums.reshape(-1, 3), m, n, "MMDu2").reshape(nb, P)
    else:
        cmp_stat, cmp_null = stat, null
    p = permutation_p_value(cmp_stat, cmp_null)
    thr = permutation_threshold(cmp_stat, cmp_null, alpha)
    if estimator == "mmd":
        with np.errstate(invalid="ignore"):
            thr = np.sqrt(thr)
    return dict(statistic=stat, null=null, p_value=p, threshold=thr, p_holm=holm_adjust(p))


def mmd_permutation_test(x, y, blocks, permutations: int = 999, seed=0, estimator: str = "MMDb", sigma=None, scale=None,
                         circular=None, alpha: float = 0.05, labels=None, device=None) -> dict:
    """What the values of `mmd_blocks` are worth: the permutation test of H0 "x and y come from one law", per block.  The two
    sets are pooled and relabelled `permutations` times (`permutation_labels(m, n, permutations, seed)`; an explicit `labels`
    bool [P, m + n] overrides `seed`), and the p-value is how often the relabelled statistic reaches the observed one:
    exact under exchangeability, one reference set is enough, valid for every estimator.  All blocks and all permutations in
    one device launch per 256-permutation-aligned chunk (nfisam_hip.mmd_perm_sums: every Gram value once, not once per
    permutation); the observed statistic comes from the `mmd_sums` launch and is `mmd_blocks`' value bit for bit.

    x, y, blocks, estimator, sigma, scale, circular, device: as `mmd_blocks`, with its checks and defaults.
    -> dict: statistic [nb], null [nb, P], p_value [nb] = (1 + #{null >= statistic}) / (1 + P) ("mmd": compared on the
    MMDu2 values), threshold [nb] (the (1 - alpha) quantile of the null with the observed value included), p_holm [nb]
    (Holm's adjustment over the blocks), permutations, seed (None with explicit labels), estimator, m, n."""
    import nfisam_hip as _nh
    table, xcols, ycols, sc, wr, m, n = _mmd_block_tables(x, y, blocks, estimator, sigma, scale, circular)
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1), got %r" % (alpha,))
    if labels is None:
        labels = permutation_labels(m, n, permutations, seed)
    else:
        labels, seed = np.asarray(labels), None
        if labels.dtype != np.bool_ or labels.ndim != 2:
            raise ValueError("labels must be a bool [permutations, m + n] array")
    _nh.check_perm_labels(labels, m, n, labels.shape[0])
    obs = _nh.mmd_sums(x, y, table, xcols, ycols, scale=sc, wrap=wr, device=device)
    null = _nh.mmd_perm_sums(x, y, table, xcols, ycols, labels, scale=sc, wrap=wr, device=device)
    out = permutation_test_from_sums(obs.cpu().numpy(), null.cpu().numpy(), m, n, estimator, alpha)
    out.update(permutations=int(labels.shape[0]), seed=seed, estimator=estimator, m=m, n=n)
    return out


# ---- how far apart two sample sets are, in their own units: sliced Wasserstein (nfisam_sample_sliced_transport) ------------------
def transport_directions(d: int, count: int, seed: int = 0) -> np.ndarray:
    """[count, d] float64 unit vectors: Gaussian rows from `np.random.default_rng([seed, d])`, normalised; d = 1 gives the
    single direction [[1.0]] whatever `count` is.  THE CONTRACT: a block's directions depend on (seed, d) alone -- not on the
    block's place in a table, nor on what else is compared -- so a block's sliced distance is the same number wherever it is
    asked for, and the first k rows for `count` = k are the first k rows for any larger count."""
    d, count, seed = int(d), int(count), int(seed)
    if d < 1 or count < 1 or seed < 0:
        raise ValueError("transport_directions: d >= 1, count >= 1 and seed >= 0 are required, got %d, %d, %d" % (d, count, seed))
    if d == 1:
        return np.ones((1, 1))
    g = np.random.default_rng([seed, d]).standard_normal((count, d))
    return g / np.sqrt((g * g).sum(1))[:, None]


def wasserstein_from_slices(slices, p: int):
    """(sliced distance, max-sliced distance) from a block's slices W_p^p (`nfisam_hip.sliced_transport`): mean^(1/p) and
    max^(1/p), in the units of the projected keys.  A NaN slice makes both NaN."""
    if p not in (1, 2):
        raise ValueError("p must be 1 or 2, got %r" % (p,))
    s = np.asarray(slices, dtype=np.float64).reshape(-1)
    if s.size < 1:
        raise ValueError("no slices")
    if np.isnan(s).any():
        return float("nan"), float("nan")
    return float(s.mean() ** (1.0 / p)), float(s.max() ** (1.0 / p))


def check_transport_options(p=2, directions=64, seed=0, m=None, n=None):
    """ValueError unless p is 1 or 2, 1 <= directions <= 65535, seed is an integer >= 0 and (where given) both sets have
    1 .. TRANSPORT_MAX_N points."""
    import nfisam_hip as _nh
    if p not in (1, 2):
        raise ValueError("p must be 1 or 2, got %r" % (p,))
    if not isinstance(directions, (int, np.integer)) or not 1 <= int(directions) <= 65535:
        raise ValueError("directions must be an integer in 1..65535, got %r" % (directions,))
    if not isinstance(seed, (int, np.integer)) or int(seed) < 0:
        raise ValueError("seed must be an integer >= 0, got %r" % (seed,))
    for name, k in (("m", m), ("n", n)):
        if k is not None and not 1 <= int(k) <= _nh.TRANSPORT_MAX_N:
            raise ValueError("%s = %d points: a set holds 1..%d (both key lists are sorted in LDS)" % (name, int(k), _nh.TRANSPORT_MAX_N))


def transport_entries(pairs, flags):
    """[(xcols, ycols)] and the circular flags of x's columns -> [(xrows, yrows, kind)]: a column becomes one entry of kind 0,
    a circular column two entries that name it, its cosine (kind 1) and its sine (kind 2) -- the chord embedding."""
    out = []
    for xc, yc in pairs:
        xr, yr, kd = [], [], []
        for a, b in zip(xc.tolist(), yc.tolist()):
            kinds = (1, 2) if flags[a] else (0,)
            xr += [a] * len(kinds); yr += [b] * len(kinds); kd += kinds
        out.append((np.asarray(xr, dtype=np.int64), np.asarray(yr, dtype=np.int64), np.asarray(kd, dtype=np.uint8)))
    return out


def transport_tables(entries, directions: int, seed: int, axes, scale=None) -> dict:
    """The tables of one launch for the blocks `entries` ([(xrows, yrows, kind)]): block b gets
    `transport_directions(its entries, directions, seed)`; for a block with `axes` (one flag, or one per block) every entry is
    also a one-entry block of its own with the direction [1.0] -- a basis vector: the exact 1-D distance of that entry --
    appended to the table and reading the block's own entries.  scale [rows of x] or None.
    -> dict: blocks (TRANSPORT_BLOCK_DTYPE), xcols, ycols, kind (None when every entry is a value), scale (per entry or
    None), dirs, main (number of blocks asked for), axis_at ({block: index of its first one-entry block})."""
    import nfisam_hip as _nh
    axes = [bool(axes)] * len(entries) if np.ndim(axes) == 0 else [bool(a) for a in axes]
    if len(axes) != len(entries):
        raise ValueError("axes: one flag, or one per block (%d), got %d" % (len(entries), len(axes)))
    dims = [int(e[0].size) for e in entries]
    cache, dirs, nd = {}, [], []
    for d in dims:
        if d not in cache:
            cache[d] = transport_directions(d, directions, seed)
        dirs.append(cache[d].reshape(-1))
        nd.append(cache[d].shape[0])
    extra = sum(d for d, a in zip(dims, axes) if a)
    if len(entries) + extra > 65535:
        raise ValueError("%d blocks and %d axis entries: a launch holds at most 65535 blocks" % (len(entries), extra))
    table = _nh.pack_transport_blocks(dims + [1] * extra, nd + [1] * extra)
    axis_at, k = {}, len(entries)
    for b, (d, a) in enumerate(zip(dims, axes)):
        if a:
            axis_at[b] = k
            table["col_off"][k:k + d] = int(table["col_off"][b]) + np.arange(d)
            k += d
    xcols = np.concatenate([e[0] for e in entries]).astype(np.int32)
    ycols = np.concatenate([e[1] for e in entries]).astype(np.int32)
    kind = np.concatenate([e[2] for e in entries]).astype(np.uint8)
    return dict(blocks=table, xcols=xcols, ycols=ycols, kind=kind if kind.any() else None,
                scale=None if scale is None else np.asarray(scale, dtype=np.float64)[xcols],
                dirs=np.concatenate(dirs + [np.ones(extra)]), main=len(entries), axis_at=axis_at)


def transport_result(out, tab: dict, p: int) -> dict:
    """The slices `out` of a launch over `transport_tables` -> dict: distance [main], max_sliced [main], slices (list of
    arrays of W_p^p), axis (list: None, or the exact 1-D W_p of every entry of the block)."""
    out = np.asarray(out, dtype=np.float64)
    t = tab["blocks"]
    slices = [out[int(t["out_off"][b]):int(t["out_off"][b]) + int(t["n_dirs"][b])].copy() for b in range(tab["main"])]
    both = [wasserstein_from_slices(s, p) for s in slices]
    axis = []
    for b in range(tab["main"]):
        k = tab["axis_at"].get(b)
        axis.append(None if k is None else out[t["out_off"][k:k + int(t["d"][b])]] ** (1.0 / p))
    return dict(distance=np.array([v[0] for v in both]), max_sliced=np.array([v[1] for v in both]), slices=slices, axis=axis)


def _transport_front(x_width, y_width, m, n, blocks, p, directions, seed, scale, circular, axes):
    """The checks of `sliced_wasserstein` and `sliced_wasserstein_t`, none of which needs a device -> the launch's tables."""
    check_transport_options(p, directions, seed, m, n)
    pairs = _block_pairs(blocks)
    for b, (xc, yc) in enumerate(pairs):
        if xc.min() < 0 or xc.max() >= x_width or yc.min() < 0 or yc.max() >= y_width:
            raise ValueError("block %d names a column outside its sample set" % b)
    flags = _column_flags(circular, x_width)
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64).reshape(-1)
        if scale.size != x_width or not np.all(np.isfinite(scale)):
            raise ValueError("scale: one finite value per column of x (%d), got %d" % (x_width, scale.size))
    return transport_tables(transport_entries(pairs, flags), int(directions), int(seed), axes, scale)


def sliced_wasserstein_t(Xt, Yt, blocks, p=2, directions=64, seed=0, scale=None, circular=None, axes=False, checked=False) -> dict:
    """`sliced_wasserstein` on the COLUMN-major device matrices Xt [x_cols, m], Yt [y_cols, n] (contiguous float32, used in
    place: what the tree walk wrote); a column is a row of them.  `checked`: `blocks` is what `transport_tables` returned."""
    import nfisam_hip as _nh
    if checked:
        tab = blocks
    else:
        if not hasattr(Xt, "shape") or not hasattr(Yt, "shape") or len(Xt.shape) != 2 or len(Yt.shape) != 2:
            raise ValueError("Xt and Yt must be [columns, points]")
        tab = _transport_front(int(Xt.shape[0]), int(Yt.shape[0]), int(Xt.shape[1]), int(Yt.shape[1]), blocks, p, directions, seed,
                               scale, circular, axes)
    out = _nh.sliced_transport_t(Xt, Yt, tab["blocks"], tab["xcols"], tab["ycols"], tab["dirs"], p, tab["kind"], tab["scale"])
    return transport_result(out.cpu().numpy(), tab, p)


def sliced_wasserstein(x, y, blocks, p=2, directions=64, seed=0, scale=None, circular=None, axes=False, device=None) -> dict:
    """The sliced Wasserstein distance W_p between the sample sets x [m, x_cols] and y [n, y_cols] (numpy or torch) restricted
    to each of `blocks`, all blocks and directions in ONE device launch (nfisam_hip.sliced_transport: float32 points, float64
    keys): how far, in the columns' own units, x must be moved to become y.  It needs no bandwidth, keeps growing with the
    separation where the MMD saturates, and sees a missing mode as mass times distance.

    blocks: as `mmd_blocks` takes them (column lists, or (xcols, ycols) pairs).  p: 1 or 2.  A block of d entries is
    projected on `transport_directions(d, directions, seed)` -- the directions depend on (seed, d) alone; a one-entry block
    has the single direction 1 and its value is the exact 1-D distance.  scale [x_cols]: factor on a column's values (and its
    partner's in y).  circular [x_cols]: columns that are angles; each becomes two entries, its cosine and its sine (the
    chord embedding: continuous across +-pi, the radian difference for small differences).  axes: also the exact 1-D W_p of
    every entry of every block (basis-vector directions, in the same launch).  At most 8192 points per set.
    -> dict: distance [n_blocks] = (mean of the slices)^(1/p), max_sliced [n_blocks] = (max of the slices)^(1/p), slices
    (list of arrays: W_p^p per direction), axis (list: None, or with `axes` the per-entry distances).  There is no CPU path."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2 or np.ndim(y) != 2:
        raise ValueError("x and y must be [points, columns]")
    tab = _transport_front(int(x.shape[1]), int(y.shape[1]), int(x.shape[0]), int(y.shape[0]), blocks, p, directions, seed, scale,
                           circular, axes)
    out = _nh.sliced_transport(x, y, tab["blocks"], tab["xcols"], tab["ycols"], tab["dirs"], p, tab["kind"], tab["scale"],
                               device=device)
    return transport_result(out.cpu().numpy(), tab, p)


# ---- what a sample set says: means, covariances, quantiles on the device (nfisam_sample_moments / nfisam_sample_quantiles) ----
def _column_blocks(blocks, width):
    out = []
    for k, b in enumerate(blocks):
        c = np.asarray(b, dtype=np.int64)
        if c.ndim != 1 or c.size < 1:
            raise ValueError("block %d: a block is a non-empty list of columns" % k)
        if c.size > 16:
            raise ValueError("block %d: %d columns; a block holds at most 16 (assemble wider matrices from pair blocks)" % (k, c.size))
        if c.min() < 0 or c.max() >= width:
            raise ValueError("block %d names a column outside the %d columns of the sample set" % (k, width))
        out.append(c)
    if not out:
        raise ValueError("no blocks")
    return out


def _column_flags(circular, width):
    if circular is None:
        return np.zeros(width, dtype=bool)
    circular = np.asarray(circular, dtype=bool).reshape(-1)
    if circular.size != width:
        raise ValueError("circular: one flag per column of x (%d), got %d" % (width, circular.size))
    return circular


def sample_moments(x, blocks, circular=None, weights=None, device=None):
    """Mean, covariance and resultant length of the sample set x [n, x_cols] (numpy or torch) restricted to each of `blocks`
    (lists of at most 16 column indices), all blocks in ONE device call (nfisam_hip.sample_moments: float32 points, float64
    arithmetic, two passes) -> list of (mean [d], cov [d, d], resultant [d]) float64 numpy arrays, one per block.

    circular [x_cols]: columns that are angles -- their mean is the circular mean in [-pi, pi) (scipy's
    circmean(high=pi, low=-pi), what the reference's `sample_mean` calls), their residuals are wrapped into [-pi, pi), and
    `resultant` holds their mean resultant length (NaN for the other columns).  cov is the population form (divided by the
    sum of the weights); for an angle, the mean squared wrapped deviation about the circular mean.  weights [n]: non-negative,
    None for all ones.  There is no CPU path."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    cols = _column_blocks(blocks, int(x.shape[1]))
    flags = _column_flags(circular, int(x.shape[1]))
    flat = np.concatenate(cols)
    table = _nh.pack_moment_blocks([c.size for c in cols])
    mean, res, cov = _nh.sample_moments(x, table, flat, circular=flags[flat].astype(np.uint8) if flags.any() else None,
                                        weights=weights, device=device)
    mean, res, cov = mean.cpu().numpy(), res.cpu().numpy(), cov.cpu().numpy()
    out = []
    for row in table:
        o, d, c = int(row["col_off"]), int(row["d"]), int(row["cov_off"])
        out.append((mean[o:o + d], cov[c:c + d * d].reshape(d, d), res[o:o + d]))
    return out


def sample_quantiles(x, probs, circular=None, device=None) -> np.ndarray:
    """Quantiles at `probs` of every column of x [n, x_cols] (numpy or torch; n <= 16384), numpy's "linear" rule on float64
    keys, sorted on the device (nfisam_hip.sample_quantiles) -> [n_probs, x_cols] float64.
    circular [x_cols]: an angle's quantiles are those of its deviations from its circular mean, wrapped into [-pi, pi), added
    back to that mean and NOT wrapped again: the ends of an interval stay ordered and may lie beyond +-pi -- wrap for display."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    width = int(x.shape[1])
    flags = _column_flags(circular, width)
    cols = np.arange(width)
    center = circ = None
    if flags.any():
        circ = flags.astype(np.uint8)
        mean, _, _ = _nh.sample_moments(x, _nh.pack_moment_blocks(np.ones(width, dtype=np.int64)), cols, circular=circ, device=device)
        center = mean                                              # (on the device; a Euclidean column's centre is not read)
    q = _nh.sample_quantiles(x, cols, probs, circular=circ, center=center, device=device)
    return q.cpu().numpy().T.copy()


# ---- which hypotheses a sample set holds: mean-shift modes on the device (nfisam_sample_modes) ---------------------------------
def effective_sample_size(weights, n: int) -> float:
    """(sum w)^2 / sum w^2 of non-negative weights (numpy, or a torch tensor: reduced where it lies); n for None."""
    if weights is None:
        return float(n)
    if hasattr(weights, "is_cuda"):
        w = weights.double()
        return float((w.sum() ** 2 / (w * w).sum()).item())
    w = np.asarray(weights, dtype=np.float64)
    return float(w.sum() ** 2 / (w * w).sum())


def mode_scale(variance, resultant, circular) -> np.ndarray:
    """The factor on a column's differences that standardises it: 1 / spread, with spread the population standard deviation
    sqrt(variance) of a Euclidean column and the circular standard deviation sqrt(-2 ln R) of an angle (R its mean resultant
    length); 0 where the spread is 0 (or not finite: R = 0): the column is ignored in distances and stays where it is."""
    variance, resultant = np.asarray(variance, dtype=np.float64), np.asarray(resultant, dtype=np.float64)
    circular = np.asarray(circular, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        spread = np.where(circular, np.sqrt(np.maximum(-2.0 * np.log(np.where(circular, resultant, 1.0)), 0.0)),
                          np.sqrt(np.maximum(variance, 0.0)))
        return np.where((spread > 0) & np.isfinite(spread), 1.0 / spread, 0.0)


def mode_sigma(n_eff: float, dims) -> np.ndarray:
    """Scott's rule on standardised columns: sigma_b = n_eff^(-1 / (d_b + 4))."""
    return float(n_eff) ** (-1.0 / (np.asarray(dims, dtype=np.float64) + 4.0))


def check_mode_options(n_blocks, width, sigma, scale, tol, merge, max_iters, max_modes):
    """ValueError for a bad sigma (one positive bandwidth, or one per block), scale (one finite value >= 0 per column) or
    scalar argument -> (sigma [n_blocks] or None, scale [width] or None)."""
    import nfisam_hip as _nh
    _nh.check_mode_args(max_iters, tol, merge, max_modes)
    if sigma is not None:
        sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(-1), (n_blocks,)).copy() if np.size(sigma) == 1 else \
            np.asarray(sigma, dtype=np.float64).reshape(-1)
        if sigma.size != n_blocks or not np.all(np.isfinite(sigma) & (sigma > 0)):
            raise ValueError("sigma is one positive bandwidth, or one per block (%d)" % n_blocks)
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64).reshape(-1)
        if scale.size != width or not np.all(np.isfinite(scale)) or np.any(scale < 0):
            raise ValueError("scale: one finite value >= 0 per column of x (%d)" % width)
    return sigma, scale


def sample_modes_t(Xt, blocks, circular=None, weights=None, sigma=None, scale=None, tol=1e-7, merge=1e-2, max_iters=500,
                   max_modes=16, checked=False) -> dict:
    """`sample_modes` on the COLUMN-major device matrix Xt [x_cols, n] (contiguous float32, used in place: what the tree walk
    wrote); `blocks` name rows of Xt, `circular` and `scale` have one value per row, `weights` is None, numpy or a device
    tensor.  `checked`: the caller has made every check (blocks, options, weights), none is repeated.  `labels` stay on the
    device."""
    import nfisam_hip as _nh
    width, n = int(Xt.shape[0]), int(Xt.shape[1])
    if n < 1:
        raise ValueError("sample_modes: no points")
    if checked:
        cols = [np.asarray(b, dtype=np.int64) for b in blocks]
        flags = np.zeros(width, dtype=bool) if circular is None else np.asarray(circular, dtype=bool).reshape(-1)
        sigma = None if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(-1), (len(cols),)).copy()
        scale = None if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    else:
        cols = _column_blocks(blocks, width)
        flags = _column_flags(circular, width)
        sigma, scale = check_mode_options(len(cols), width, sigma, scale, tol, merge, max_iters, max_modes)
        weights = _nh._check_weights(weights, n)
    flat = np.concatenate(cols)
    dims = np.array([c.size for c in cols])
    n_eff = effective_sample_size(weights, n)
    if scale is None:
        used = np.unique(flat)
        mean, res, cov = _nh.sample_moments_t(Xt, _nh.pack_moment_blocks(np.ones(used.size, dtype=np.int64)), used,
                                              flags[used].astype(np.uint8) if flags[used].any() else None, weights, checked=True)
        scale = np.zeros(width)
        scale[used] = mode_scale(cov.cpu().numpy(), res.cpu().numpy(), flags[used])
    if sigma is None:
        sigma = mode_sigma(n_eff, dims)
    table = _nh.pack_mmd_blocks(dims, sigma)
    wrap = flags[flat].astype(np.uint8)
    raw = _nh.sample_modes_t(Xt, table, flat, scale[flat], wrap if wrap.any() else None, weights, tol, merge, max_iters, max_modes,
                             checked=True)
    n_modes = raw["n_modes"].cpu().numpy()
    mpos, mdens, mmass = raw["mode_pos"].cpu().numpy(), raw["mode_dens"].cpu().numpy(), raw["mode_mass"].cpu().numpy()
    its = raw["iters"]
    modes = [[dict(position=mpos[b, m, :int(dims[b])].copy(), mass=float(mmass[b, m]), density=float(mdens[b, m]))
              for m in range(int(n_modes[b]))] for b in range(len(cols))]
    return dict(modes=modes, labels=raw["labels"],
                iterations=dict(max=its.abs().max(dim=1).values.cpu().numpy(), not_converged=(its < 0).sum(dim=1).cpu().numpy()),
                unlabelled=raw["unlabelled"].cpu().numpy(), sigma=np.asarray(sigma, dtype=np.float64), scale=scale, n_eff=n_eff,
                raw=raw)


def sample_modes(x, blocks, circular=None, weights=None, sigma=None, scale=None, tol=1e-7, merge=1e-2, max_iters=500, max_modes=16,
                 device=None) -> dict:
    """The modes of the sample set x [n, x_cols] (numpy or torch) restricted to each of `blocks` (lists of at most 16 column
    indices): from every point a mean-shift ascent on the block's Gaussian kernel density estimate, then a deterministic merge
    of the converged points -- all blocks in ONE device call (nfisam_hip.sample_modes_t: float32 points, float64 arithmetic).

    circular [x_cols]: columns that are angles (differences wrapped into [-pi, pi): a mode may sit across the +-pi seam).
    weights [n]: non-negative, None for all ones.  scale [x_cols]: the factor on a column's differences; None: 1 / spread, the
    weighted population standard deviation of the column from `nfisam_hip.sample_moments_t` (the circular standard deviation
    sqrt(-2 ln R) of an angle), 0 for a column without spread, which is then ignored in distances and keeps its value exactly.
    sigma: one bandwidth or one per block, in those standardised units; None: Scott's rule n_eff^(-1 / (d + 4)) with
    n_eff = (sum w)^2 / sum w^2.  tol, merge: in sigmas: an ascent stops at a shift of at most `tol`, converged points within
    `merge` of a mode join it (keep merge well above tol * r / (1 - r), r the slowest ascent's contraction per iteration -- 1e-5
    sigma at the default tol on a flat density --: members of one mode end that far apart).  At most max_modes (<= 32) modes per
    block, by falling density.  The rule finds every bump of the density estimate: a near-Gaussian sample of some hundred points
    has small ones in its tails, so read `mass` before counting hypotheses, and `iterations` for ascents that did not converge.
    -> dict: modes (per block a list of {position [d], mass, density}), labels ([n_blocks, n] int32, -1 for a point left over
    when max_modes was reached; left on the device when x was a device tensor), iterations ({max, not_converged}: per block),
    unlabelled (per block), sigma (per block), scale (per column), n_eff, raw (the device tensors of nfisam_hip.sample_modes_t).
    Every ValueError is raised before anything is launched.  There is no CPU path."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    n, width = int(x.shape[0]), int(x.shape[1])
    if n < 1:
        raise ValueError("sample_modes: no points")
    cols = _column_blocks(blocks, width)
    flags = _column_flags(circular, width)
    sigma, scale = check_mode_options(len(cols), width, sigma, scale, tol, merge, max_iters, max_modes)
    weights = _nh._check_weights(weights, n)
    on_device = hasattr(x, "is_cuda") and x.is_cuda
    if device is None:
        device = x.device if on_device else "cuda"
    out = sample_modes_t(_nh._columns(x, device), cols, flags, weights, sigma, scale, tol, merge, max_iters, max_modes,
                         checked=True)
    if not on_device:
        out["labels"] = out["labels"].cpu().numpy()
    return out


# ---- how uncertain, how coupled: k-nearest-neighbour entropy, mutual information, divergence (nfisam_sample_knn) -------------
EULER_GAMMA = 0.57721566490153286061


def digamma_table(n: int) -> np.ndarray:
    """psi(j) for j = 1 .. n as a float64 table t[j] (t[0] is NaN), by psi(1) = -gamma, psi(j + 1) = psi(j) + 1 / j.  The
    running sum carries its rounding error along (Neumaier's compensation), so every entry is the float64 nearest to the sum
    of the ROUNDED terms up to O(n u^2): within u (|psi(j)| + H_(j-1) / 2) of psi(j), not the n u / 2 of a plain recurrence."""
    t = np.full(int(n) + 1, np.nan)
    s, c = -EULER_GAMMA, 0.0
    for j in range(1, int(n) + 1):
        t[j] = s + c
        term = 1.0 / j
        r = s + term
        c += (s - r) + term if abs(s) >= term else (term - r) + s
        s = r
    return t


@functools.lru_cache(maxsize=8)
def _psi(n: int) -> np.ndarray:
    """`digamma_table(n)`, kept and read-only: the estimators ask for the same n block after block."""
    t = digamma_table(n)
    t.setflags(write=False)
    return t


def knn_log_unit_ball(d, norm: str):
    """log of the volume of the unit ball of `norm` in d dimensions: d log 2 (max), (d / 2) log pi - lgamma(d / 2 + 1) (l2)."""
    d = np.asarray(d, dtype=np.float64)
    if norm == "max":
        return d * math.log(2.0)
    if norm == "l2":
        return 0.5 * d * math.log(math.pi) - np.vectorize(math.lgamma)(0.5 * d + 1.0)
    raise ValueError("norm must be 'max' or 'l2', got %r" % (norm,))


def entropy_from_log_sum(log_sum, n_used, d, k: int, norm: str = "max", log_scale_sum=0.0) -> np.ndarray:
    """Kozachenko-Leonenko, per block, on the host:
        H = psi(n_used) - psi(k) + log c_d + (d / n_used) * log_sum - log_scale_sum
    with log_sum the sum of log(eps_i) over the n_used queries whose k-th neighbour distance eps_i (a RADIUS, in the scaled
    coordinates) is positive and finite, c_d the unit ball's volume and log_scale_sum = sum_e log scale_e, which brings the
    entropy back to the original units.  NaN where n_used = 0.  -> float64 [n_blocks] nats."""
    log_sum, ls = np.atleast_1d(np.asarray(log_sum, dtype=np.float64)), np.asarray(log_scale_sum, dtype=np.float64)
    nu, d = np.atleast_1d(np.asarray(n_used, dtype=np.int64)), np.asarray(d, dtype=np.float64)
    psi = _psi(max(int(nu.max(initial=1)), int(k), 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        h = psi[np.maximum(nu, 0)] - psi[int(k)] + knn_log_unit_ball(d, norm) + (d / nu) * log_sum - ls
    return np.where(nu > 0, h, np.nan)


def ksg_from_counts(n_a, n_b, k: int) -> float:
    """Kraskov-Stoegbauer-Grassberger estimator 1 on the host: I = psi(k) + psi(n) - mean_i[psi(n_a_i + 1) + psi(n_b_i + 1)],
    n_a_i / n_b_i the number of OTHER points strictly inside eps_i (the k-th max-norm distance in the joint space) in either
    marginal space; psi from `digamma_table`, the 2 n terms added by math.fsum.  -> nats."""
    n_a, n_b = np.asarray(n_a, dtype=np.int64).reshape(-1), np.asarray(n_b, dtype=np.int64).reshape(-1)
    n = int(n_a.size)
    if n < 1 or n_b.size != n or min(int(n_a.min()), int(n_b.min())) < 0:
        raise ValueError("n_a and n_b are two lists of n >= 1 counts >= 0")
    psi = _psi(max(int(n_a.max()) + 1, int(n_b.max()) + 1, n, int(k)))
    return psi[int(k)] + psi[n] - math.fsum(np.concatenate([psi[n_a + 1], psi[n_b + 1]]).tolist()) / n


def check_knn_options(width, k=4, norm="max", scale=None, m=None, n=None, norms=("max", "l2")):
    """ValueError for a bad k (an integer in 1..16), norm (one of `norms`), scale (one finite value >= 0 per column) or too few
    points (a query needs k neighbours: m > k within one set, n >= k in another) -> scale [width] or None."""
    import nfisam_hip as _nh
    if norm not in norms:
        raise ValueError("norm must be %s, got %r" % (" or ".join(repr(v) for v in norms), norm))
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _nh.KNN_MAX_K:
        raise ValueError("k must be an integer in 1..%d, got %r" % (_nh.KNN_MAX_K, k))
    if m is not None and m <= int(k):
        raise ValueError("%d points have no %d-th neighbour among themselves (more than k points are needed)" % (m, int(k)))
    if n is not None and n < int(k):
        raise ValueError("%d points hold no %d-th neighbour (at least k points are needed)" % (n, int(k)))
    if scale is not None:
        scale = np.asarray(scale, dtype=np.float64).reshape(-1)
        if scale.size != width or not np.all(np.isfinite(scale)) or np.any(scale < 0):
            raise ValueError("scale: one finite value >= 0 per column of x (%d)" % width)
    return scale


def _knn_scale(Xt, used, flags, scale, width):
    """scale [width]: the given one, or `mode_scale` of the columns `used` from nfisam_hip.sample_moments_t (0 elsewhere)."""
    import nfisam_hip as _nh
    if scale is not None:
        return np.asarray(scale, dtype=np.float64).reshape(-1)
    used = np.unique(used)
    mean, res, cov = _nh.sample_moments_t(Xt, _nh.pack_moment_blocks(np.ones(used.size, dtype=np.int64)), used,
                                          flags[used].astype(np.uint8) if flags[used].any() else None, None, checked=True)
    scale = np.zeros(width)
    scale[used] = mode_scale(cov.cpu().numpy(), res.cpu().numpy(), flags[used])
    return scale


def _log_scale_sums(scale, cols):
    """sum_e log scale_e per block; -inf marks a block with a column without spread."""
    with np.errstate(divide="ignore"):
        return np.array([math.fsum(np.log(scale[c]).tolist()) if np.all(scale[c] > 0) else -np.inf for c in cols])


def _knn_front(x, device):
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    if device is None:
        device = x.device if hasattr(x, "is_cuda") and x.is_cuda else "cuda"
    return device


def knn_entropy_t(Xt, blocks, k=4, circular=None, scale=None, norm="max", checked=False) -> dict:
    """`knn_entropy` on the COLUMN-major device matrix Xt [x_cols, n] (contiguous float32, used in place: what the tree walk
    wrote); `blocks` name rows of Xt, `circular` and `scale` have one value per row.  `checked`: the caller has made every
    check."""
    import nfisam_hip as _nh
    width, n = int(Xt.shape[0]), int(Xt.shape[1])
    if checked:
        cols = [np.asarray(b, dtype=np.int64) for b in blocks]
        flags = np.zeros(width, dtype=bool) if circular is None else np.asarray(circular, dtype=bool).reshape(-1)
    else:
        cols = _column_blocks(blocks, width)
        flags = _column_flags(circular, width)
        scale = check_knn_options(width, k, norm, scale, m=n)
    flat = np.concatenate(cols)
    dims = np.array([c.size for c in cols])
    scale = _knn_scale(Xt, flat, flags, scale, width)
    wrap = flags[flat].astype(np.uint8)
    raw = _nh.sample_knn_t(Xt, None, _nh.pack_knn_blocks(dims), flat, flat, int(k), norm, scale[flat], wrap if wrap.any() else None,
                           exclude_self=True, checked=True)
    n_used, log_sum = raw["n_used"].cpu().numpy(), raw["log_sum"].cpu().numpy()
    zeros = (raw["dist"][:, int(k) - 1, :] == 0).sum(dim=1).cpu().numpy()
    ls = _log_scale_sums(scale, cols)
    with np.errstate(invalid="ignore"):
        h = np.where(np.isfinite(ls), entropy_from_log_sum(log_sum, n_used, dims, int(k), norm, np.where(np.isfinite(ls), ls, 0.0)),
                     -np.inf)
    return dict(entropy=h, n_used=n_used, zeros=zeros, log_sum=log_sum, scale=scale, n=n, k=int(k), raw=raw)


def knn_entropy(x, blocks, k=4, circular=None, scale=None, norm="max", device=None) -> dict:
    """The differential entropy, in nats, of the sample set x [n, x_cols] (numpy or torch) restricted to each of `blocks` (lists
    of at most 16 column indices), by the Kozachenko-Leonenko k-nearest-neighbour estimator -- the neighbour search of all
    blocks in ONE device call (nfisam_hip.sample_knn_t: float32 points, float64 arithmetic), the formula
    (`entropy_from_log_sum`) on the host.  Unlike 1/2 log det(2 pi e Sigma) it stays meaningful on a ring or on two modes.

    circular [x_cols]: columns that are angles (differences wrapped into [-pi, pi)).  scale [x_cols]: the factor on a column's
    differences; None: 1 / spread from `nfisam_hip.sample_moments_t` (`mode_scale`: standardised coordinates); the estimate is
    brought back to the original units by - sum log scale.  A block with a column without spread (scale 0) has entropy -inf.
    norm: "max" or "l2".  Queries whose k-th distance is 0 (duplicated points) are left out and counted in `zeros`; a block
    without a usable query gives NaN.  The estimator is consistent, not exact: at n = 2000, k = 4 it is within some 0.05 nats.
    -> dict: entropy [n_blocks], n_used [n_blocks], zeros [n_blocks], log_sum [n_blocks], scale [x_cols], n, k, raw (the
    device tensors of nfisam_hip.sample_knn_t).  Every ValueError is raised before anything is launched.  No CPU path."""
    import nfisam_hip as _nh
    device = _knn_front(x, device)
    n, width = int(x.shape[0]), int(x.shape[1])
    cols = _column_blocks(blocks, width)
    flags = _column_flags(circular, width)
    scale = check_knn_options(width, k, norm, scale, m=n)
    return knn_entropy_t(_nh._columns(x, device), cols, k, flags, scale, norm, checked=True)


def _pair_blocks(pairs_of_blocks, width):
    out = []
    for p, pair in enumerate(pairs_of_blocks):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError("pair %d: a pair is (columns of A, columns of B)" % p)
        a, b = _column_blocks(pair, width)
        if a.size + b.size > 16:
            raise ValueError("pair %d: %d columns; a joint block holds at most 16" % (p, a.size + b.size))
        out.append((a, b))
    if not out:
        raise ValueError("no pairs")
    return out


def knn_mutual_information_t(Xt, pairs_of_blocks, k=4, circular=None, scale=None, norm="max", checked=False) -> dict:
    """`knn_mutual_information` on the COLUMN-major device matrix Xt [x_cols, n]; see `knn_entropy_t`."""
    import nfisam_hip as _nh
    width, n = int(Xt.shape[0]), int(Xt.shape[1])
    if checked:
        pairs = [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in pairs_of_blocks]
        flags = np.zeros(width, dtype=bool) if circular is None else np.asarray(circular, dtype=bool).reshape(-1)
    else:
        pairs = _pair_blocks(pairs_of_blocks, width)
        flags = _column_flags(circular, width)
        scale = check_knn_options(width, k, norm, scale, m=n, norms=("max",))
    joint = [np.concatenate(p) for p in pairs]
    flat = np.concatenate(joint)
    scale = _knn_scale(Xt, flat, flags, scale, width)
    wrap = flags[flat].astype(np.uint8)
    raw = _nh.sample_knn_t(Xt, None, _nh.pack_knn_blocks([c.size for c in joint]), flat, flat, int(k), "max", scale[flat],
                           wrap if wrap.any() else None, exclude_self=True, checked=True)
    eps = raw["dist"][:, int(k) - 1, :].contiguous()
    sides = [c for p in pairs for c in p]                          # A and B of pair p: blocks 2 p and 2 p + 1, radius row p
    sflat = np.concatenate(sides)
    swrap = flags[sflat].astype(np.uint8)
    count = _nh.sample_ball_count_t(Xt, None, _nh.pack_knn_blocks([c.size for c in sides], np.repeat(np.arange(len(pairs)), 2)),
                                    sflat, sflat, eps, "max", scale[sflat], swrap if swrap.any() else None, exclude_self=True,
                                    checked=True)
    cnt = count.cpu().numpy()
    mi = np.array([ksg_from_counts(cnt[2 * p], cnt[2 * p + 1], int(k)) for p in range(len(pairs))])
    return dict(mi=mi, zeros=(eps == 0).sum(dim=1).cpu().numpy(), scale=scale, n=n, k=int(k), raw=dict(raw, eps=eps, count=count))


def knn_mutual_information(x, pairs_of_blocks, k=4, circular=None, scale=None, norm="max", device=None) -> dict:
    """The mutual information, in nats, between the column blocks A and B of each pair of `pairs_of_blocks` ([(columns of A,
    columns of B)], at most 16 columns together) over the sample set x [n, x_cols], by estimator 1 of Kraskov, Stoegbauer and
    Grassberger: eps_i is the k-th max-norm distance of point i in the joint block (nfisam_hip.sample_knn_t), n_a_i and n_b_i
    count the other points strictly inside eps_i in A and in B (nfisam_hip.sample_ball_count_t), and `ksg_from_counts` forms
    I = psi(k) + psi(n) - mean[psi(n_a + 1) + psi(n_b + 1)] on the host.  Only the max norm is accepted.  circular, scale: as
    `knn_entropy` (the information does not depend on a column's scale; standardising keeps a wide column from deciding every
    distance).  The estimate of independent blocks scatters about 0 and can be slightly negative.
    -> dict: mi [n_pairs], zeros [n_pairs] (points whose eps is 0), scale, n, k, raw."""
    import nfisam_hip as _nh
    device = _knn_front(x, device)
    n, width = int(x.shape[0]), int(x.shape[1])
    pairs = _pair_blocks(pairs_of_blocks, width)
    flags = _column_flags(circular, width)
    scale = check_knn_options(width, k, norm, scale, m=n, norms=("max",))
    return knn_mutual_information_t(_nh._columns(x, device), pairs, k, flags, scale, checked=True)


def divergence_from_log_sums(log_sum_nu, log_sum_rho, used_nu, used_rho, d, m: int, n: int) -> np.ndarray:
    """Wang-Kulkarni-Verdu on the host, per block: D = (d / m) (log_sum_nu - log_sum_rho) + log(n / (m - 1)); NaN unless every
    one of the m queries was used on both sides."""
    d = np.asarray(d, dtype=np.float64)
    ok = (np.asarray(used_nu) == m) & (np.asarray(used_rho) == m)
    val = (d / m) * (np.asarray(log_sum_nu, dtype=np.float64) - np.asarray(log_sum_rho, dtype=np.float64)) + math.log(n / (m - 1.0))
    return np.where(ok, val, np.nan)


def knn_divergence_t(Xt, Yt, blocks, k=4, circular=None, scale=None, norm="max", checked=False) -> dict:
    """`knn_divergence` on the COLUMN-major device matrices Xt [x_cols, m], Yt [y_cols, n]; `blocks`: [(rows of Xt, rows of
    Yt)]; circular and scale have one value per row of Xt."""
    import nfisam_hip as _nh
    width, m, n = int(Xt.shape[0]), int(Xt.shape[1]), int(Yt.shape[1])
    if checked:
        pairs = [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in blocks]
        flags = np.zeros(width, dtype=bool) if circular is None else np.asarray(circular, dtype=bool).reshape(-1)
    else:
        pairs = _divergence_blocks(blocks, width, int(Yt.shape[0]))
        flags = _column_flags(circular, width)
        scale = check_knn_options(width, k, norm, scale, m=m, n=n)
    xc, yc = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    dims = np.array([p[0].size for p in pairs])
    scale = _knn_scale(Xt, xc, flags, scale, width)
    wrap = flags[xc].astype(np.uint8)
    wrap = wrap if wrap.any() else None
    table = _nh.pack_knn_blocks(dims)
    rho = _nh.sample_knn_t(Xt, None, table, xc, xc, int(k), norm, scale[xc], wrap, exclude_self=True, checked=True)
    nu = _nh.sample_knn_t(Xt, Yt, table, xc, yc, int(k), norm, scale[xc], wrap, exclude_self=False, checked=True)
    used = [r["n_used"].cpu().numpy() for r in (nu, rho)]
    div = divergence_from_log_sums(nu["log_sum"].cpu().numpy(), rho["log_sum"].cpu().numpy(), used[0], used[1], dims, m, n)
    return dict(divergence=div, n_used=np.minimum(used[0], used[1]), scale=scale, m=m, n=n, k=int(k), raw=dict(rho=rho, nu=nu))


def _divergence_blocks(blocks, x_width, y_width):
    pairs = _block_pairs(blocks)
    for b, (xc, yc) in enumerate(pairs):
        if xc.size > 16:
            raise ValueError("block %d: %d columns; a block holds at most 16" % (b, xc.size))
        if xc.min() < 0 or xc.max() >= x_width or yc.min() < 0 or yc.max() >= y_width:
            raise ValueError("block %d names a column outside its sample set" % b)
    return pairs


def knn_divergence(x, y, blocks, k=4, circular=None, scale=None, norm="max", device=None) -> dict:
    """The Kullback-Leibler divergence D(P || Q), in nats, of the law P of the sample set x [m, x_cols] from the law Q of
    y [n, y_cols], restricted to each of `blocks` (column lists that apply to both sets, or (xcols, ycols) pairs; at most 16
    columns), by the k-nearest-neighbour estimator of Wang, Kulkarni and Verdu:
        D = (d / m) (sum_i log nu_i - sum_i log rho_i) + log(n / (m - 1)),
    rho_i the k-th distance of x_i within x (itself excluded), nu_i its k-th distance within y -- two calls of
    nfisam_hip.sample_knn_t, `divergence_from_log_sums` on the host.  NaN unless every query was used on both sides (a
    duplicated point, or a point of x that is also in y, has distance 0).  circular, scale ([x_cols]; None: standardised by
    x's spreads), norm: as `knn_entropy`; the scale cancels in D.
    -> dict: divergence [n_blocks], n_used [n_blocks], scale, m, n, k, raw."""
    import nfisam_hip as _nh
    device = _knn_front(x, device)
    if np.ndim(y) != 2:
        raise ValueError("y must be [points, columns]")
    width = int(x.shape[1])
    pairs = _divergence_blocks(blocks, width, int(y.shape[1]))
    flags = _column_flags(circular, width)
    scale = check_knn_options(width, k, norm, scale, m=int(x.shape[0]), n=int(y.shape[0]))
    return knn_divergence_t(_nh._columns(x, device), _nh._columns(y, device), pairs, k, flags, scale, norm, checked=True)


# ---- the marginal density itself, where the caller asks: a Gaussian KDE in logs on the device (nfisam_sample_density) ----------
DENSITY_RULES = ("scott", "silverman", "loo")
DENSITY_LOO_POWERS = tuple(range(-10, 3))        # leave-one-out candidates: the Scott factor times 2^(k / 2)
DENSITY_CIRCULAR_VARIANCE_CAP = math.pi ** 2 / 3.0   # the variance of a uniform heading


def density_factor(n_eff: float, d: int, rule) -> float:
    """The bandwidth factor of scipy.stats.gaussian_kde: n_eff^(-1 / (d + 4)) for "scott", (n_eff (d + 2) / 4)^(-1 / (d + 4))
    for "silverman", or `rule` itself, a positive float."""
    if isinstance(rule, str):
        if rule == "scott":
            return float(n_eff) ** (-1.0 / (d + 4.0))
        if rule == "silverman":
            return (float(n_eff) * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0))
        raise ValueError("bandwidth is 'scott', 'silverman', 'loo' or a positive factor, got %r" % (rule,))
    if isinstance(rule, bool) or not np.isscalar(rule) or not np.isfinite(rule) or not rule > 0:
        raise ValueError("bandwidth is 'scott', 'silverman', 'loo' or a positive factor, got %r" % (rule,))
    return float(rule)


def density_bandwidth(cov, n_eff: float, d: int, rule, circular=None) -> np.ndarray:
    """The bandwidth matrix H [d, d] of a Gaussian KDE, as scipy.stats.gaussian_kde forms it: `cov` -- the POPULATION covariance
    `nfisam_hip.sample_moments_t` returns, a heading's deviations wrapped -- made unbiased, cov / (1 - 1 / n_eff), times
    factor^2 (`density_factor`).  circular [d]: a circular column's variance is capped at pi^2 / 3, the variance of a uniform
    heading, before the factor (its row and column are scaled down together), so that a ring's heading keeps a kernel the
    nearest image can carry.  ValueError for a column without spread, a matrix that is not positive definite, n_eff <= 1."""
    cov = np.array(cov, dtype=np.float64).reshape(d, d)
    factor = density_factor(n_eff, d, rule)
    if not float(n_eff) > 1.0:
        raise ValueError("a bandwidth needs an effective sample size above 1, got %r" % (n_eff,))
    var = np.diag(cov)
    if not np.all(np.isfinite(cov)) or not np.all(var > 0):
        raise ValueError("a column has no spread (variances %s): it has no density" % (var,))
    if circular is not None:
        circular = np.asarray(circular, dtype=bool).reshape(-1)
        shrink = np.where(circular & (var > DENSITY_CIRCULAR_VARIANCE_CAP), np.sqrt(DENSITY_CIRCULAR_VARIANCE_CAP / var), 1.0)
        cov = cov * shrink[:, None] * shrink[None, :]
    return cov / (1.0 - 1.0 / float(n_eff)) * factor ** 2


def density_whiten(H) -> np.ndarray:
    """W = inv(cholesky(H)): lower triangular with W H W' = I.  ValueError when H is not positive definite."""
    H = np.asarray(H, dtype=np.float64)
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        raise ValueError("the bandwidth matrix is not positive definite (columns without joint spread)") from None
    W = np.linalg.solve(L, np.eye(L.shape[0]))
    return np.tril(W)


def hpd_level(log_dens_samples, log_dens_point, weights=None):
    """The credible level of the smallest highest-density region that contains a point: the (weighted) share of the samples
    whose own KDE log density is at least the point's.  Near 0: the point sits on the peak; near 1: in the tails; over many
    calibrated posteriors it is uniform.  log_dens_samples [n], log_dens_point: a scalar or [q]; weights [n] or None.  Torch
    tensors are reduced where they lie (-> a tensor of log_dens_point's shape), anything else with numpy."""
    if hasattr(log_dens_samples, "is_cuda"):
        import torch
        s = log_dens_samples.double().reshape(-1)
        p = torch.as_tensor(log_dens_point, dtype=torch.float64, device=s.device)
        w = torch.ones_like(s) if weights is None else torch.as_tensor(weights, dtype=torch.float64, device=s.device).reshape(-1)
        inside = (s[None, :] >= p.reshape(-1, 1)).to(torch.float64)
        return ((inside * w[None, :]).sum(dim=1) / w.sum()).reshape(p.shape)
    s = np.asarray(log_dens_samples, dtype=np.float64).reshape(-1)
    p = np.asarray(log_dens_point, dtype=np.float64)
    w = np.ones_like(s) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    inside = (s[None, :] >= p.reshape(-1, 1)).astype(np.float64)
    out = ((inside * w[None, :]).sum(axis=1) / w.sum()).reshape(p.shape)
    return float(out) if out.ndim == 0 else out


def check_density_options(bandwidth, n: int, m: int = None, exclude_self=False):
    """ValueError for a bad bandwidth rule or too few points (two at least: the unbiased covariance; leave-one-out)."""
    if isinstance(bandwidth, str):
        if bandwidth not in DENSITY_RULES:
            raise ValueError("bandwidth is 'scott', 'silverman', 'loo' or a positive factor, got %r" % (bandwidth,))
    else:
        density_factor(2.0, 1, bandwidth)
    if n < 2:
        raise ValueError("a density estimate needs at least two samples, got %d" % n)
    if exclude_self and m is not None and m != n:
        raise ValueError("exclude_self needs the queries to be the samples (m = %d, n = %d)" % (m, n))


def _density_blocks(blocks, x_width, q_width):
    import nfisam_hip as _nh
    pairs = _block_pairs(blocks)
    for b, (xc, qc) in enumerate(pairs):
        if xc.size > _nh.DENSITY_MAX_D:
            raise ValueError("block %d: %d columns; a density block holds at most %d" % (b, xc.size, _nh.DENSITY_MAX_D))
        if xc.min() < 0 or xc.max() >= x_width or qc.min() < 0 or qc.max() >= q_width:
            raise ValueError("block %d names a column outside its matrix" % b)
    return pairs


def _loo_mean(log_dens, weights):
    """The (weighted) mean over the samples of every row of log_dens [rows, n], on the device; a zero weight's row entry is
    not read."""
    if weights is None:
        return log_dens.mean(dim=1)
    import torch
    w = torch.as_tensor(weights, dtype=torch.float64, device=log_dens.device)
    return torch.where(w[None, :] > 0, log_dens * w[None, :], torch.zeros_like(log_dens)).sum(dim=1) / w.sum()


def density_bandwidths_t(Xt, cols, flags, weights=None, bandwidth="scott") -> dict:
    """The bandwidth of every block `cols` (lists of rows of the COLUMN-major device matrix Xt [x_cols, n]; flags: which rows
    are angles): the blocks' covariances from ONE nfisam_hip.sample_moments_t call, `density_bandwidth` on the host.
    "loo": every (block, candidate) pair -- the Scott factor times 2^(k / 2), k = -10 .. 2 -- is one block of ONE
    nfisam_hip.sample_density_t launch with the samples as queries and exclude_self; the largest (weighted) mean
    leave-one-out log density picks the factor, the lowest candidate on ties.  A candidate too wide for a heading (pi / 3) is
    left out.  Arguments are taken as checked.
    -> dict: H (list of [d, d]), W (their whitening matrices), factor [n_blocks], n_eff, loo (None, or per block {factors,
    scores})."""
    import nfisam_hip as _nh
    n = int(Xt.shape[1])
    n_eff = effective_sample_size(weights, n)
    flat = np.concatenate(cols)
    dims = np.array([c.size for c in cols])
    wrap = flags[flat].astype(np.uint8)
    table = _nh.pack_moment_blocks(dims)
    _, _, cov = _nh.sample_moments_t(Xt, table, flat, wrap if wrap.any() else None, weights, checked=True)
    cov = cov.cpu().numpy()
    covs = [cov[int(r["cov_off"]):int(r["cov_off"]) + int(r["d"]) ** 2].reshape(int(r["d"]), int(r["d"])) for r in table]
    circ = [flags[c] for c in cols]
    loo = None
    if bandwidth == "loo":
        cand, owner, Ws, offs = [], [], [], []
        for b, (c, d) in enumerate(zip(cols, dims)):
            scott = density_factor(n_eff, int(d), "scott")
            for k in DENSITY_LOO_POWERS:
                f = scott * 2.0 ** (k / 2.0)
                W = density_whiten(density_bandwidth(covs[b], n_eff, int(d), f, circ[b]))
                if np.any(circ[b] & (1.0 / np.diag(W) > _nh.DENSITY_MAX_WIDTH)):
                    continue
                cand.append(f), owner.append(b), Ws.append(W), offs.append(int(table["col_off"][b]))
            if b not in owner:
                raise ValueError("block %d: every leave-one-out candidate is too wide for its heading" % b)
        owner = np.asarray(owner)
        blocks = _nh.pack_density_blocks(dims[owner], Ws, offs)
        wr = wrap if wrap.any() else None
        _nh.check_density_blocks(blocks, flat, flat, int(Xt.shape[0]), int(Xt.shape[0]), wr)
        res = _nh.sample_density_t(Xt, None, blocks, flat, flat, wr, None, True, False, checked=True, weights=weights)
        scores = _loo_mean(res["log_density"], weights).cpu().numpy()
        cand = np.asarray(cand)
        factor, loo = np.zeros(len(cols)), []
        for b in range(len(cols)):
            mine = np.flatnonzero(owner == b)
            s = np.where(np.isnan(scores[mine]), -np.inf, scores[mine])
            factor[b] = cand[mine][int(np.argmax(s))]                    # (the first maximum: the lowest candidate on ties)
            loo.append(dict(factors=cand[mine].copy(), scores=scores[mine].copy()))
    else:
        factor = np.array([density_factor(n_eff, int(d), bandwidth) for d in dims])
    H = [density_bandwidth(covs[b], n_eff, int(dims[b]), float(factor[b]), circ[b]) for b in range(len(cols))]
    return dict(H=H, W=[density_whiten(h) for h in H], factor=factor, n_eff=n_eff, loo=loo)


def sample_density_t(Xt, Qt, blocks, circular=None, weights=None, bandwidth="scott", exclude_self=False, want_density=False,
                     checked=False) -> dict:
    """`sample_density` on the COLUMN-major device matrices Xt [x_cols, n] (the samples) and Qt [q_cols, m] (the queries; None:
    the samples themselves) -- contiguous float32, used in place: what the tree walk wrote.  `blocks`: lists of rows (of both
    matrices) or (rows of Xt, rows of Qt) pairs; circular has one flag per row of Xt.  `checked`: the caller has made every
    check.  The results stay on the device."""
    import nfisam_hip as _nh
    width, n = int(Xt.shape[0]), int(Xt.shape[1])
    q_width, m = (width, n) if Qt is None else (int(Qt.shape[0]), int(Qt.shape[1]))
    if checked:
        pairs = [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in _block_pairs(blocks)]
        flags = np.zeros(width, dtype=bool) if circular is None else np.asarray(circular, dtype=bool).reshape(-1)
    else:
        pairs = _density_blocks(blocks, width, q_width)
        flags = _column_flags(circular, width)
        check_density_options(bandwidth, n, m, exclude_self)
        weights = _nh._check_weights(weights, n)
    cols = [p[0] for p in pairs]
    bw = density_bandwidths_t(Xt, cols, flags, weights, bandwidth)
    xc, qc = np.concatenate(cols), np.concatenate([p[1] for p in pairs])
    wrap = flags[xc].astype(np.uint8)
    wrap = wrap if wrap.any() else None
    table = _nh.pack_density_blocks([c.size for c in cols], bw["W"])
    _nh.check_density_blocks(table, qc, xc, q_width, width, wrap)
    res = _nh.sample_density_t(Xt if Qt is None else Qt, Xt, table, qc, xc, wrap, None, exclude_self, want_density, checked=True,
                               weights=weights)
    out = dict(log_density=res["log_density"], factor=bw["factor"], H=bw["H"], n_eff=bw["n_eff"])
    if want_density:
        out["density"] = res["density"]
    if bw["loo"] is not None:
        out["loo"] = bw["loo"]
    return out


def sample_density(x, queries, blocks, circular=None, weights=None, bandwidth="scott", exclude_self=False, want_density=False,
                   device=None) -> dict:
    """The Gaussian kernel density estimate of the sample set x [n, x_cols] (numpy or torch) at the rows of `queries`
    [m, q_cols] (None: the samples themselves), restricted to each of `blocks` (lists of at most 6 column indices that apply to
    both, or (columns of x, columns of queries) pairs), in logs -- what scipy.stats.gaussian_kde(x[:, block].T).logpdf
    returns, for all blocks in ONE device call (nfisam_hip.sample_density_t: float32 points, float64 arithmetic, a full
    bandwidth matrix per block).

    circular [x_cols]: columns that are angles (differences wrapped into [-pi, pi); the nearest image alone is summed, so a
    heading's kernel may be at most pi / 3 wide).  weights [n]: non-negative, None for all ones.  bandwidth: "scott",
    "silverman" or a positive factor -- scipy's rules on the unbiased (weighted) covariance (`density_bandwidth`) -- or "loo":
    the factor among the Scott factor times 2^(k / 2), k = -10 .. 2, with the largest mean leave-one-out log density (one more
    launch).  On a ring or on two hypotheses Scott's rule is several times too wide; "loo" is not.  exclude_self: the
    leave-one-out density (queries None).
    -> dict: log_density [n_blocks, m] (a float64 device tensor), density (the same, with want_density), factor [n_blocks],
    H (per block [d, d]), n_eff, and with "loo": loo (per block {factors, scores}).  Every ValueError -- a bad block, rule
    or weight, fewer than two samples, a column without spread -- is raised before the density launch.  No CPU path."""
    import nfisam_hip as _nh
    device = _knn_front(x, device)
    if queries is not None and np.ndim(queries) != 2:
        raise ValueError("queries must be [points, columns]")
    n, width = int(x.shape[0]), int(x.shape[1])
    m, q_width = (n, width) if queries is None else (int(queries.shape[0]), int(queries.shape[1]))
    pairs = _density_blocks(blocks, width, q_width)
    flags = _column_flags(circular, width)
    check_density_options(bandwidth, n, m, exclude_self)
    if m < 1:
        raise ValueError("no queries")
    weights = _nh._check_weights(weights, n)
    return sample_density_t(_nh._columns(x, device), None if queries is None else _nh._columns(queries, device), pairs, flags,
                            weights, bandwidth, exclude_self, want_density, checked=True)


# ---- trajectory error of every sample: aligned ATE and RPE on the device (nfisam_sample_trajectory_error / _rpe) ---------------
def trajectory_entries(width, truth_xy, truth_th=None, pose_cols=None, landmark_cols=None, landmark_xy=None):
    """The entry table of `trajectory_error` for a sample set of `width` columns: P poses, time-ordered, graded against
    truth_xy [P, 2] (and truth_th [P] where they have headings), then L landmarks against landmark_xy [L, 2], outside the
    alignment.  pose_cols [P, 3] (or [P, 2] without headings) names their columns; default: consecutive triples (pairs
    without truth_th) from column 0.  landmark_cols [L, 2]; default with landmark_xy: consecutive pairs after the poses.
    -> (numpy TRAJ_ENTRY_DTYPE table, P)."""
    import nfisam_hip as _nh
    xy = np.asarray(truth_xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
        raise ValueError("truth_xy must be [poses, 2] with at least one pose, got %s" % (xy.shape,))
    P = xy.shape[0]
    d = 2 if truth_th is None else 3
    if truth_th is not None and np.shape(truth_th) != (P,):
        raise ValueError("truth_th must be [%d], got %s" % (P, np.shape(truth_th)))
    pc = np.arange(P * d).reshape(P, d) if pose_cols is None else np.asarray(pose_cols, dtype=np.int64)
    if pc.ndim != 2 or pc.shape != (P, d):
        raise ValueError("pose_cols must be [%d, %d], got %s" % (P, d, pc.shape))
    L = 0
    if landmark_xy is not None or landmark_cols is not None:
        if landmark_xy is None:
            raise ValueError("landmark_cols needs landmark_xy, the landmarks' ground truth")
        lxy = np.asarray(landmark_xy, dtype=np.float64)
        if lxy.ndim != 2 or lxy.shape[1] != 2:
            raise ValueError("landmark_xy must be [landmarks, 2], got %s" % (lxy.shape,))
        L = lxy.shape[0]
        lc = int(pc.max()) + 1 + np.arange(L * 2).reshape(L, 2) if landmark_cols is None else np.asarray(landmark_cols, dtype=np.int64)
        if lc.shape != (L, 2):
            raise ValueError("landmark_cols must be [%d, 2], got %s" % (L, lc.shape))
        xy = np.vstack([xy, lxy])
        pc = np.vstack([np.hstack([pc, np.full((P, 3 - d), -1)]), np.hstack([lc, np.full((L, 1), -1)])])
        d = 3
    th = None if truth_th is None else np.concatenate([np.asarray(truth_th, dtype=np.float64), np.zeros(L)])
    entries = _nh.pack_traj_entries(pc[:, 0], pc[:, 1], pc[:, 2] if d == 3 else np.full(P + L, -1), xy, th,
                                    landmark=np.arange(P + L) >= P)
    _nh.check_traj_entries(entries, int(width), "none")
    return entries, P


def _trajectory_result(r) -> dict:
    """The device dict of nfisam_hip.sample_trajectory_error_t -> host float64 arrays in the words of `trajectory_error`."""
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    nt, nl, nh_ = host["n_traj"], host["n_landmark"], host["n_heading"]
    W = float(host["weight_sum"])
    nan = np.full_like(host["sse_traj"], np.nan)
    per_entry = np.sqrt(host["entry_sums"] / W)
    return dict(ate=np.sqrt(host["sse_traj"] / nt) if nt else nan, heading_rms=np.sqrt(host["sse_heading"] / nh_) if nh_ else nan,
                landmark_rmse=np.sqrt(host["sse_landmark"] / nl) if nl else nan, theta=host["theta"], scale=host["scale"],
                t=host["t"].T.copy(), reflected=host["reflected"].astype(bool), worst_pose=(host["worst_entry"], host["worst"]),
                per_entry_rmse=per_entry, weight_sum=W, n=int(host["theta"].size))


def trajectory_error_t(Xt, entries, align="rigid", reflect=False, weights=None, checked=False) -> dict:
    """`trajectory_error` on the COLUMN-major float32 device matrix Xt [x_rows, n] (used in place) and a packed entry table
    (`trajectory_entries`, or nfisam_hip.pack_traj_entries: its rows name rows of Xt)."""
    import nfisam_hip as _nh
    return _trajectory_result(_nh.sample_trajectory_error_t(Xt, entries, align, reflect, weights, checked=checked))


def trajectory_error(x, truth_xy, truth_th=None, pose_cols=None, landmark_cols=None, landmark_xy=None, align="rigid",
                     reflect=False, weights=None, device=None) -> dict:
    """The absolute trajectory error of EVERY row of the sample set x [n, x_cols] (numpy or torch) against ground truth, each
    row aligned to the truth on its own, in one device call (nfisam_hip.sample_trajectory_error: float32 points, float64
    arithmetic, the planar Kabsch-Umeyama fit in closed form) -- what the reference's Plaza scripts do for the posterior mean
    alone with `kabsch_umeyama` on the host.  The columns and truths are those of `trajectory_entries`.
    align: "none", "rigid" (rotation and translation) or "similarity" (and the least-squares scale g / sum |b'|^2 -- not the
    scale rule of utils.Functions.kabsch_umeyama); reflect: also try the mirrored fit.  Landmarks are graded through the
    poses' transform and take no part in it.  weights [n] enter per_entry_rmse alone.
    -> dict of float64 numpy arrays: ate, heading_rms, landmark_rmse [n] (root mean squares over the poses, their headings,
    the landmarks; NaN where there are none), theta, scale [n], t [n, 2], reflected [n] bool, worst_pose ((entry [n], its
    residual [n]): the pose farthest from its truth), per_entry_rmse [P + L] (sqrt(sum_i w_i |r_e,i|^2 / sum_i w_i): which
    stretch of the path is off), weight_sum, n.  A row with a NaN or infinite coordinate has NaN results, and
    per_entry_rmse with it.  There is no CPU path."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    entries, _ = trajectory_entries(int(x.shape[1]), truth_xy, truth_th, pose_cols, landmark_cols, landmark_xy)
    return _trajectory_result(_nh.sample_trajectory_error(x, entries, align, reflect, weights, device=device))


def _rpe_result(r, strides) -> dict:
    trans, rot, count = r["trans"].cpu().numpy(), r["rot"].cpu().numpy(), r["count"]
    return {int(k): dict(trans=np.sqrt(trans[s] / count[s]), rot=np.sqrt(rot[s] / count[s]), pairs=int(count[s]))
            for s, k in enumerate(strides)}


def check_strides(strides, poses: int):
    """-> the tuple of strides; ValueError unless it is a non-empty list of distinct integers in [1, poses)."""
    try:
        out = tuple(int(k) for k in strides)
        exact = all(float(k) == int(k) for k in strides)
    except (TypeError, ValueError):
        raise ValueError("strides is a list of integers, got %r" % (strides,)) from None
    if not out or not exact or len(set(out)) != len(out):
        raise ValueError("strides is a non-empty list of distinct integers, got %r" % (strides,))
    for k in out:
        if not 1 <= k < poses:
            raise ValueError("stride %d: a stride lies in [1, %d) for %d poses" % (k, poses, poses))
    return out


def relative_pose_error_t(Xt, entries, poses, strides=(1,), checked=False) -> dict:
    """`relative_pose_error` on the COLUMN-major device matrix Xt and a packed entry table; `poses`: the time-ordered entries."""
    import nfisam_hip as _nh
    strides = check_strides(strides, len(poses))
    pairs = _nh.pack_traj_pairs(poses, strides)
    n_slots = _nh.check_traj_pairs(pairs, entries, len(strides))
    if not checked:
        _nh.check_traj_entries(entries, int(Xt.shape[0]), "none")
    return _rpe_result(_nh.sample_trajectory_rpe_t(Xt, entries, pairs, n_slots, checked=True), strides)


def relative_pose_error(x, truth_xy, truth_th, pose_cols=None, strides=(1,), device=None) -> dict:
    """Relative pose error of every row of x [n, x_cols] over the time-ordered poses of `trajectory_entries`: for the poses k
    and k + stride, d = R(-th_k) (p_{k+stride} - p_k) and dth = wrap_pi(th_{k+stride} - th_k) from the sample and from the truth;
    gauge-free, so nothing is aligned (nfisam_hip.sample_trajectory_rpe, every stride in one launch).
    -> {stride: dict(trans [n], rot [n], pairs)}: the root mean squares of |d_est - d_true| and of
    wrap_pi(dth_est - dth_true) over the stride's pairs, float64 numpy."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    if truth_th is None:
        raise ValueError("relative_pose_error needs headings: truth_th")
    entries, P = trajectory_entries(int(x.shape[1]), truth_xy, truth_th, pose_cols)
    strides = check_strides(strides, P)
    pairs = _nh.pack_traj_pairs(np.arange(P), strides)
    return _rpe_result(_nh.sample_trajectory_rpe(x, entries, pairs, len(strides), device=device), strides)


def weighted_quantiles(values, probs, weights=None) -> np.ndarray:
    """Quantiles of `values` at `probs`: numpy's "linear" rule without weights; with weights the inverted weighted CDF -- the
    smallest value whose cumulative weight reaches p times the total."""
    v = np.asarray(values, dtype=np.float64)
    p = np.asarray(probs, dtype=np.float64).reshape(-1)
    if weights is None:
        return np.quantile(v, p)
    order = np.argsort(v, kind="stable")
    cum = np.cumsum(np.asarray(weights, dtype=np.float64)[order])
    at = np.minimum(np.searchsorted(cum, p * cum[-1], side="left"), v.size - 1)
    return v[order][at]


def trajectory_error_summary(ate, weights=None, quantiles=(0.05, 0.5, 0.95), threshold=None) -> dict:
    """What the per-sample errors `ate` [n] say, on the host in float64 (n numbers need no kernel): -> dict(mean (weighted),
    quantiles ({p: value}, `weighted_quantiles`), best (sample, value), below (the share of the weight on samples with
    ate < threshold; None without a threshold), ess ((sum w)^2 / sum w^2), n, n_nan).  Samples whose error is NaN carry no
    weight here and are counted in n_nan."""
    a = np.asarray(ate, dtype=np.float64).reshape(-1)
    if a.size < 1:
        raise ValueError("trajectory_error_summary: no samples")
    probs = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    if not np.all((probs >= 0.0) & (probs <= 1.0)):
        raise ValueError("quantiles is a list of probabilities in [0, 1]")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size != a.size or not np.all(np.isfinite(w)) or np.any(w < 0) or not np.any(w > 0):
            raise ValueError("weights must be [n] = [%d], finite, non-negative and not all zero" % a.size)
    ok = np.isfinite(a)
    if w is not None:
        ok &= w > 0
    if not ok.any():
        return dict(mean=float("nan"), quantiles={float(p): float("nan") for p in probs}, best=(-1, float("nan")),
                    below=None if threshold is None else float("nan"), ess=0.0, n=int(a.size), n_nan=int((~np.isfinite(a)).sum()))
    av, wv = a[ok], (np.ones(int(ok.sum())) if w is None else w[ok])
    q = weighted_quantiles(av, probs, None if w is None else wv)
    best = int(np.flatnonzero(ok)[np.argmin(av)])
    return dict(mean=float(np.sum(wv * av) / np.sum(wv)), quantiles={float(p): float(v) for p, v in zip(probs, q)},
                best=(best, float(a[best])), below=None if threshold is None else float(np.sum(wv[av < threshold]) / np.sum(wv)),
                ess=float(np.sum(wv) ** 2 / np.sum(wv * wv)), n=int(a.size), n_nan=int((~np.isfinite(a)).sum()))


def sample_mean(samples, var_ordering):
    """The reference's `sample_mean` (src/utils/Statistics.py:151-171) on the device: the mean of every column of samples
    [n, sum of the variables' dims], circular for the columns the variables flag as angles, arithmetic for the others
    -> (means [columns], {variable: its slice of means})."""
    import nfisam_hip as _nh
    flags = np.array([bool(c) for v in var_ordering for c in v.circular_dim_list], dtype=bool)
    if np.ndim(samples) != 2 or int(samples.shape[1]) != flags.size:
        raise ValueError("samples must be [n, %d] for these variables" % flags.size)
    width = flags.size
    mean, _, _ = _nh.sample_moments(samples, _nh.pack_moment_blocks(np.ones(width, dtype=np.int64)), np.arange(width),
                                    circular=flags.astype(np.uint8) if flags.any() else None)
    means = mean.cpu().numpy()
    var2mean, at = {}, 0
    for v in var_ordering:
        var2mean[v] = means[at:at + v.dim]
        at += v.dim
    return means, var2mean


def rmse(samples1: np.ndarray, samples2: np.ndarray) -> float:
    """Root of the mean squared elementwise difference of two equally shaped arrays (reference: :142-148)."""
    a, b = np.asarray(samples1), np.asarray(samples2)
    if a.shape != b.shape:
        raise ValueError("the two sample sets differ in shape: %s and %s" % (a.shape, b.shape))
    diff = a - b
    return np.sqrt(np.sum(diff ** 2) / a.size)


def _planar(var):
    from slam.Variables import R2Variable, SE2Variable
    if isinstance(var, SE2Variable):
        return "SE2"
    if isinstance(var, R2Variable):
        return "R2"
    raise ValueError("Unknown variable type: %r" % (var,))


def translation_terms(var2point1, var2point2) -> dict:
    """variable -> squared distance between the xy parts of its two points (the terms `translation_distance` averages)."""
    terms = {}
    for var in var2point1:
        _planar(var)
        a, b = np.asarray(var2point1[var]), np.asarray(var2point2[var])
        terms[var] = sum((a[:2] - b[:2]) ** 2)
    return terms


def translation_distance(var2point1, var2point2):
    """sqrt of the mean over the variables of the squared xy distance between two assignments (reference: :204-214): the
    trajectory RMSE the run scripts report."""
    terms = translation_terms(var2point1, var2point2)
    err = 0
    for var in var2point1:
        err += terms[var]
    return np.sqrt(err / len(var2point1))


def geodesic_distance(var2point1, var2point2):
    """sqrt of the summed squared geodesic distances between two assignments (reference: :179-191): |Log(p1 p2^-1)|^2 for a
    pose (geometry.TwoDimension.SE2Pose), |p1 - p2|^2 for a point."""
    from geometry.TwoDimension import SE2Pose
    err = 0
    for var in var2point1:
        a, b = var2point1[var], var2point2[var]
        if _planar(var) == "SE2":
            err += sum((SE2Pose(*a) / SE2Pose(*b)).log_map() ** 2)
        else:
            err += sum((np.asarray(a) - np.asarray(b)) ** 2)
    return np.sqrt(err)


# ---- kernel Stein discrepancy: samples graded against the factor graph itself (nfisam_sample_ksd) ---------------------------------
def ksd_from_sums(row_sum: float, diag_sum: float, n: int, ustat: bool = True):
    """(ustat, vstat) of the Stein sums: vstat = sum_ij h_ij / n^2 (all pairs), ustat = (sum_ij h_ij - sum_i h_ii) / (n (n - 1))
    (reference src/utils/Statistics.py:237-238).  `row_sum` = sum of `row`, `diag_sum` = sum of `diag` of `nfisam_hip.ksd_sums`.
    The U-statistic needs n >= 2 (ValueError); with ustat=False it is returned as None."""
    n = int(n)
    if n < 1:
        raise ValueError("the Stein sums need at least one point")
    if ustat and n < 2:
        raise ValueError("the U-statistic needs at least two points (n = %d)" % n)
    v = float(row_sum) / (n * n)
    u = (float(row_sum) - float(diag_sum)) / (n * (n - 1)) if ustat else None
    return u, v


def _diagonal_precision(kernel_precision, dim):
    """A [D] vector or a DIAGONAL [D, D] matrix -> the [D] diagonal; any other dense matrix is refused."""
    p = np.asarray(kernel_precision, dtype=np.float64)
    if p.ndim == 2 and p.shape == (dim, dim):
        if np.any(p != np.diag(np.diag(p))):
            raise ValueError("kernel_precision is a dense matrix with off-diagonal entries: only a diagonal precision "
                             "(a [D] vector or a diagonal [D, D] matrix) is supported")
        p = np.diag(p).copy()
    if p.shape != (dim,):
        raise ValueError("kernel_precision must be a [%d] vector or a diagonal [%d, %d] matrix, got shape %s"
                         % (dim, dim, dim, tuple(p.shape)))
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        raise ValueError("kernel_precision must be finite and >= 0")
    return p


def ksd_bootstrap(H, draws) -> np.ndarray:
    """The reference's bootstrap of the U-statistic (src/utils/Statistics.py:239-242): for every row c of the multinomial
    counts `draws` [nboot, n], w = c / n and (w - 1/n)' off (w - 1/n) with `off` = H without its diagonal.  H: the [n, n]
    float64 device matrix of `ksd_sums(matrix=True)`; one matrix product on its device.  -> [nboot] float64 numpy."""
    import torch
    n = int(H.shape[0])
    draws = np.asarray(draws, dtype=np.float64)
    if draws.ndim != 2 or draws.shape[1] != n:
        raise ValueError("draws must be [nboot, %d] multinomial counts" % n)
    W = torch.from_numpy(draws / n - 1.0 / n).to(H.device)
    off = H - torch.diag(torch.diagonal(H))
    return ((W @ off) * W).sum(1).cpu().numpy()


def kernel_stein_discrepancy(x, score, sigma=None, scale=None, circular=None, nboot=0, rng=None, matrix=False, device=None):
    """The Gaussian kernel Stein discrepancy of the points x [n, D] (numpy or torch; float32 points) with scores
    score [n, D] = grad_x log p at them (float64; `nfisam_hip.factor_graph_score`, `NFiSAM.joint_score`), on the device
    (nfisam_hip.ksd_sums: float64 arithmetic, direct differences) -- it grades the samples against the density itself and
    needs no second sample set.

    The kernel is exp(-1/2 sum_c p_c d_c^2) with the diagonal precision p_c = scale_c^2 / sigma^2; sigma=None means sqrt(D),
    the default of `mmd_blocks`; scale=None means all ones (scale_c = 1 / spread of column c standardises the columns; 0
    takes a column out of the kernel).  circular [D]: columns that are angles, compared by differences wrapped into
    [-pi, pi].  For a circular column the kernel is continuous but not differentiable at the antipode, where its value is
    exp(-1/2 p pi^2): negligible for concentrated headings.  The reference does not wrap: pass circular=None for its
    behaviour.

    -> dict: "ustat" (None for n = 1), "vstat", "row" [n] (row means sum_j h_ij / n: where the samples disagree with the
    density), "precision" [D]; with matrix=True "H" [n, n] (numpy, n <= 4096); with nboot > 0 (n >= 2, n <= 4096):
    "bootstrap" [nboot], the reference's multinomial bootstrap with draws from `rng` (numpy Generator or RandomState; default
    np.random) on the host and the quadratic forms as one matrix product on the device, and "p_value", the share >= ustat."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2 or np.ndim(score) != 2:
        raise ValueError("x and score must be [points, columns]")
    n, D = int(x.shape[0]), int(x.shape[1])
    if tuple(score.shape) != (n, D):
        raise ValueError("score must have the shape of x, %s, got %s" % ((n, D), tuple(score.shape)))
    if n < 1 or D < 1:
        raise ValueError("at least one point and one column are needed")
    sig = float(np.sqrt(D)) if sigma is None else float(sigma)
    if not np.isfinite(sig) or sig <= 0:
        raise ValueError("sigma must be positive and finite")
    sc = np.ones(D) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    if sc.size != D:
        raise ValueError("scale: one value per column (%d), got %d" % (D, sc.size))
    if not np.all(np.isfinite(sc)):
        raise ValueError("scale must be finite")
    wr = None
    if circular is not None:
        wr = np.asarray(circular, dtype=bool).reshape(-1)
        if wr.size != D:
            raise ValueError("circular: one flag per column (%d), got %d" % (D, wr.size))
    nboot = int(nboot)
    if nboot < 0:
        raise ValueError("nboot must be >= 0")
    if nboot > 0 and n < 2:
        raise ValueError("the bootstrap of the U-statistic needs at least two points")
    precision = sc * sc / (sig * sig)
    want_h = bool(matrix) or nboot > 0
    sums = _nh.ksd_sums(x, score, precision, wrap=wr, matrix=want_h, device=device)
    row = sums["row"].cpu().numpy()
    u, v = ksd_from_sums(row.sum(), sums["diag"].cpu().numpy().sum(), n, ustat=n >= 2)
    out = dict(ustat=u, vstat=v, row=row / n, precision=precision)
    if matrix:
        out["H"] = sums["H"].cpu().numpy()
    if nboot > 0:
        draw = (rng if rng is not None else np.random).multinomial
        draws = np.stack([draw(n, np.ones(n) / n) for _ in range(nboot)])
        out["bootstrap"] = ksd_bootstrap(sums["H"], draws)
        out["p_value"] = float(np.mean(out["bootstrap"] >= u))
    return out


def Gaussian_kernel_stein_discrepancy(joint_factor_or_score, kernel_precision, samples, nboot=10, rng=None, device=None):
    """The reference's function of this name (src/utils/Statistics.py:216-245) -> (ustats, p_u, off_ksd, vstats), the pairwise
    sums on the device.  The first argument is the [n, D] score matrix at `samples`, or any object with
    `grad_x_log_pdf(samples)`; kernel_precision a [D] vector or a DIAGONAL [D, D] matrix (any other dense matrix raises
    ValueError).  off_ksd [n, n] numpy: h_ij with a zero diagonal; p_u: the share of the `nboot` multinomial bootstrap values
    (drawn from `rng`, default np.random like the reference) that are >= ustats.  Differences are not wrapped, as there.
    Nothing is printed."""
    import nfisam_hip as _nh
    if np.ndim(samples) != 2:
        raise ValueError("samples must be [points, columns]")
    n, D = int(samples.shape[0]), int(samples.shape[1])
    precision = _diagonal_precision(kernel_precision, D)
    if n < 2:
        raise ValueError("the U-statistic needs at least two points (n = %d)" % n)
    nboot = int(nboot)
    if nboot < 1:
        raise ValueError("nboot must be >= 1")
    score = joint_factor_or_score.grad_x_log_pdf(np.asarray(samples, dtype=np.float64)) \
        if hasattr(joint_factor_or_score, "grad_x_log_pdf") else joint_factor_or_score
    if np.ndim(score) != 2 or tuple(score.shape) != (n, D):
        raise ValueError("the score must have the shape of samples, %s" % ((n, D),))
    sums = _nh.ksd_sums(samples, score, precision, matrix=True, device=device)
    ustats, vstats = ksd_from_sums(sums["row"].cpu().numpy().sum(), sums["diag"].cpu().numpy().sum(), n)
    draw = (rng if rng is not None else np.random).multinomial
    draws = np.stack([draw(n, np.ones(n) / n) for _ in range(nboot)])
    boot = ksd_bootstrap(sums["H"], draws)
    off = sums["H"].cpu().numpy()
    np.fill_diagonal(off, 0.0)
    return ustats, float(np.mean(boot >= ustats)), off, vstats


# ---- the samples moved along the score: Stein variational refinement and plain ascent (nfisam_sample_svgd / _step) ------------
def check_refine_options(width, blocks, sigma=None, scale=None, circular=None, steps=0, step_size=1.0, alpha=0.9, fudge=1e-6):
    """Every option of the Stein variational functions, checked with no device: `blocks` a non-empty list of non-empty column
    lists of any width inside [0, width) that share no column (a column has one direction); sigma one positive bandwidth or one
    per block (None: sqrt(block width), the rule of `kernel_stein_discrepancy`); scale one finite value per column (None: ones);
    circular one flag per column; steps an integer >= 0; step_size one positive finite step or one per column; alpha in [0, 1);
    fudge positive and finite.  -> dict(cols: list of int64 arrays, flat, dims, sigma [n_blocks], scale [width], flags [width],
    step [width], steps)."""
    import nfisam_hip as _nh
    cols = []
    for k, b in enumerate(blocks):
        c = np.asarray(b, dtype=np.int64)
        if c.ndim != 1 or c.size < 1:
            raise ValueError("block %d: a block is a non-empty list of columns" % k)
        if c.min() < 0 or c.max() >= width:
            raise ValueError("block %d names a column outside the %d columns of the sample set" % (k, width))
        cols.append(c)
    if not cols:
        raise ValueError("no blocks")
    flat = np.concatenate(cols)
    if np.unique(flat).size != flat.size:
        raise ValueError("overlapping blocks: a column is named more than once, and a column has one direction")
    dims = np.array([c.size for c in cols])
    if sigma is None:
        sig = np.sqrt(dims.astype(np.float64))
    else:
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(-1), (len(cols),)).copy() if np.size(sigma) == 1 else \
            np.asarray(sigma, dtype=np.float64).reshape(-1)
        if sig.size != len(cols) or not np.all(np.isfinite(sig) & (sig > 0)):
            raise ValueError("sigma is one positive bandwidth, or one per block (%d)" % len(cols))
    sc = np.ones(width) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    if sc.size != width or not np.all(np.isfinite(sc)):
        raise ValueError("scale: one finite value per column of x (%d)" % width)
    flags = _column_flags(circular, width)
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 0:
        raise ValueError("steps must be an integer >= 0, got %r" % (steps,))
    step = np.broadcast_to(np.asarray(step_size, dtype=np.float64).reshape(-1), (width,)).copy() if np.size(step_size) == 1 else \
        np.asarray(step_size, dtype=np.float64).reshape(-1)
    if step.size != width or not np.all(np.isfinite(step) & (step > 0)):
        raise ValueError("step_size is one positive finite step, or one per column (%d)" % width)
    _nh.check_step_args(alpha, fudge)
    return dict(cols=cols, flat=flat, dims=dims, sigma=sig, scale=sc, flags=flags, step=step, steps=int(steps))


def _refine_tables(opt, device):
    """The checked options `opt` as the tables of the two bindings on `device` (one upload) -> (block table, tables)."""
    import nfisam_hip as _nh
    flat = opt["flat"]
    table = _nh.pack_mmd_blocks(opt["dims"], opt["sigma"])
    wrap = opt["flags"][flat].astype(np.uint8)
    return table, _nh.svgd_tables(device, table, flat, opt["scale"][flat], wrap if wrap.any() else None, opt["step"][flat])


def stein_variational_direction(x, score, blocks, sigma=None, scale=None, circular=None, device=None) -> np.ndarray:
    """The Stein variational direction phi(x_i) = 1/n sum_j [k(x_j, x_i) score_j + grad_{x_j} k(x_j, x_i)] of the points x [n, D]
    (numpy or torch; float32 points) with scores score [n, D] = grad_x log p at them (float64), on the device
    (nfisam_hip.svgd_direction: float64 arithmetic, direct differences): the direction in which `kernel_stein_discrepancy`
    falls fastest.  `blocks`: a list of column lists, as `sample_modes` takes them but of any width and sharing no column; each
    block's kernel exp(-sum_c (scale_c d_c)^2 / (2 sigma^2)) sees the block's own columns only.  sigma: one bandwidth or one per
    block, None = sqrt(block width); scale: per column (1 / spread standardises; 0 takes a column out of the kernel); circular
    [D]: columns that are angles, compared by differences wrapped into [-pi, pi].
    -> [n, D] float64 numpy, zero in the columns no block names.  Every ValueError is raised before anything is launched."""
    import nfisam_hip as _nh
    if np.ndim(x) != 2 or np.ndim(score) != 2:
        raise ValueError("x and score must be [points, columns]")
    n, D = int(x.shape[0]), int(x.shape[1])
    if tuple(score.shape) != (n, D):
        raise ValueError("score must have the shape of x, %s, got %s" % ((n, D), tuple(score.shape)))
    if n < 1 or D < 1:
        raise ValueError("at least one point and one column are needed")
    opt = check_refine_options(D, blocks, sigma, scale, circular)
    flat = opt["flat"]
    wrap = opt["flags"][flat].astype(np.uint8)
    Phi = _nh.svgd_direction(x, score, _nh.pack_mmd_blocks(opt["dims"], opt["sigma"]), flat, opt["scale"][flat],
                             wrap if wrap.any() else None, device=device)
    out = np.zeros((n, D))
    out[:, flat] = Phi.cpu().numpy().T
    return out


def stein_variational_refine_t(Xt, score_t, blocks, steps, step_size, sigma=None, scale=None, circular=None, kernel=True,
                               alpha=0.9, fudge=1e-6, after_step=None) -> dict:
    """Stein variational gradient descent of the particles in the COLUMN-major device matrix Xt [D, n] (contiguous float32),
    IN PLACE and entirely on the device: `steps` times Gt = score_t(Xt) (a callable Xt -> the float64 column-major device
    matrix of grad log p, e.g. around `nfisam_hip.factor_graph_score_t`), phi = `nfisam_hip.svgd_direction_t`, then
    `nfisam_hip.sample_step_t`: x += step phi / (sqrt(hist) + fudge) with hist the decayed mean of phi^2 (the AdaGrad rule
    of the original SVGD code).  blocks, sigma, scale, circular: as `stein_variational_direction`; step_size: one step length or
    one per column, in the column's own unit.  kernel=False: phi is the score itself, every particle climbs alone (a MAP ascent)
    and no pairwise launch is made.  after_step: a callable (Xt, step index) run after every step (what `map_refine` keeps its
    best iterates with).  The points stay float32: a step below a coordinate's float32 spacing (7.6e-6 at 100 m) is lost.
    -> dict(hist [n_entries, n] float64 device tensor, entries in block order; cols: the row of every entry; steps).
    steps = 0 leaves every bit alone; two runs give the same bits.  Every option is checked before anything is launched."""
    import nfisam_hip as _nh
    import torch
    if not callable(score_t):
        raise ValueError("score_t must be a callable Xt -> Gt")
    if np.ndim(Xt) != 2:
        raise ValueError("Xt must be [columns, points]")
    opt = check_refine_options(int(Xt.shape[0]), blocks, sigma, scale, circular, steps, step_size, alpha, fudge)
    D, n = _nh._column_major_front("Xt", Xt)
    if n < 1:
        raise ValueError("stein_variational_refine: no points")
    table, tables = _refine_tables(opt, Xt.device)
    hist = torch.zeros(opt["flat"].size, n, dtype=torch.float64, device=Xt.device)
    rows = tables["cols"].to(torch.int64)
    for t in range(opt["steps"]):
        Gt = score_t(Xt)
        if kernel:
            Phi = _nh.svgd_direction_t(Xt, Gt, table, opt["flat"], checked=True, tables=tables)
        else:
            _nh._score_front("the score", Gt, Xt)
            if tuple(Gt.shape) != (D, n):
                raise ValueError("the score matrix must have the shape of the points: %s, got %s" % ((D, n), tuple(Gt.shape)))
            Phi = Gt.index_select(0, rows)
        _nh.sample_step_t(Xt, None, Phi, hist, None, alpha=alpha, fudge=fudge, first=t == 0, checked=True, tables=tables)
        if after_step is not None:
            after_step(Xt, t)
    return dict(hist=hist, cols=opt["flat"], steps=opt["steps"])


def stein_variational_refine(x, score, blocks, steps, step_size, sigma=None, scale=None, circular=None, kernel=True, alpha=0.9,
                             fudge=1e-6, device=None) -> dict:
    """`stein_variational_refine_t` for row-major points x [n, D] (numpy or torch) and a score that is a callable on numpy:
    score(points [n, D] float64) -> [n, D].  The direction and the step run on the device; the score is called on the host
    once per step -- the convenience form: a device score belongs behind `stein_variational_refine_t`.
    -> dict(x [n, D] float32 numpy: the refined points, hist [n, D] float64 numpy (zero in the columns no block names), steps)."""
    import nfisam_hip as _nh
    import torch
    if not callable(score):
        raise ValueError("score must be a callable points -> scores")
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    n, D = int(x.shape[0]), int(x.shape[1])
    if n < 1 or D < 1:
        raise ValueError("at least one point and one column are needed")
    check_refine_options(D, blocks, sigma, scale, circular, steps, step_size, alpha, fudge)
    device = _nh._row_major_front("stein_variational_refine", device, x=x)
    Xt = _nh._columns(x, device)

    def score_t(Xt):
        g = np.asarray(score(Xt.t().cpu().numpy().astype(np.float64)), dtype=np.float64)
        if g.shape != (n, D):
            raise ValueError("score must return the shape of x, %s, got %s" % ((n, D), g.shape))
        return torch.from_numpy(np.ascontiguousarray(g.T)).to(Xt.device)

    res = stein_variational_refine_t(Xt, score_t, blocks, steps, step_size, sigma, scale, circular, kernel, alpha, fudge)
    hist = np.zeros((n, D))
    hist[:, res["cols"]] = res["hist"].cpu().numpy().T
    return dict(x=Xt.t().cpu().numpy().copy(), hist=hist, steps=res["steps"])


# ---- Metropolis-corrected chains: MALA / random walk with independence jumps (nfisam_sample_propose / nfisam_sample_accept) ----
METROPOLIS_TARGET = {"mala": 0.574, "rw": 0.234}                      # the optimal-scaling acceptance rates (Roberts & Rosenthal 2001)
# The accept step keeps the nearest image of the wrapped normal.  At a residual rho the next image weighs
# exp(-2 pi (pi - |rho|) / h^2) of it: below 2^-53 while |rho| <= pi - 5.85 h^2, which for h <= 0.3 rad is 2.61 rad >= 8.7 h --
# a normal draw beyond 8.7 sigma has probability 3e-18.  
WRAP_STEP_MAX = 0.3
# The blocking plateau's conventions (`blocking_tau`).  A level counts once its pooled variance of block means rests on at least
# BLOCKING_MIN_DOF degrees of freedom: the estimate's relative standard error is sqrt(2 / dof), 18 % at 64.  The estimate is called
# resolved once the longest counted block spans at least BLOCKING_PLATEAU autocorrelation times: at b = 4 tau an AR(1) chain's
# blocking estimate has reached about 1 - tau / (2 b) = 7/8 of its limit; below that the estimate is still growing with b and is
# a LOWER bound.  Both are conventions, not theorems.
BLOCKING_MIN_DOF = 64
BLOCKING_PLATEAU = 4.0
CHAIN_DEFAULT_LEVELS = 8                                              # record["levels"] = None: min(8, floor(log2 T))


def check_metropolis_options(width, steps=0, step_size=1.0, circular=None, kernel="mala", warmup=0, target_accept=None, seed=None,
                             independence=None):
    """Every option of the Metropolis functions, checked with no device: kernel "mala" or "rw"; steps an integer >= 0, warmup an
    integer in [0, steps]; step_size one finite step >= 0 or one per column, in the column's own unit (0 freezes a column), at
    most WRAP_STEP_MAX = 0.3 rad on a circular column (the nearest-image bound); circular one flag per column; target_accept in
    (0, 1) (None: 0.574 for MALA, 0.234 for the random walk); seed None or an integer in [0, 2^64); independence None or
    (every >= 1, draw_t callable), which needs every column free (no step of 0).
    -> dict(h [width], flags [width] bool, steps, warmup, kernel, target, seed, every, draw_t)."""
    if kernel not in ("mala", "rw"):
        raise ValueError("kernel must be 'mala' or 'rw', got %r" % (kernel,))
    for name, v in (("steps", steps), ("warmup", warmup)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
            raise ValueError("%s must be an integer >= 0, got %r" % (name, v))
    if int(warmup) > int(steps):
        raise ValueError("warmup (%d) counts among the steps (%d): it cannot exceed them" % (warmup, steps))
    width = int(width)
    if width < 1:
        raise ValueError("at least one column is needed")
    try:
        h = np.asarray(step_size, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("step_size is one finite step >= 0, or one per column (%d)" % width) from None
    h = np.broadcast_to(h, (width,)).copy() if h.size == 1 else h
    if h.size != width or not np.all(np.isfinite(h) & (h >= 0)):
        raise ValueError("step_size is one finite step >= 0, or one per column (%d)" % width)
    flags = _column_flags(circular, width)
    if np.any(h[flags] > WRAP_STEP_MAX):
        raise ValueError("step_size: a circular column's step is at most %g rad (the nearest-image bound), got %g"
                         % (WRAP_STEP_MAX, float(h[flags].max())))
    target = METROPOLIS_TARGET[kernel] if target_accept is None else target_accept
    if np.ndim(target) != 0 or not (np.isfinite(target) and 0.0 < target < 1.0):
        raise ValueError("target_accept must lie in (0, 1), got %r" % (target_accept,))
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64):
        raise ValueError("seed must be None or an integer in [0, 2^64), got %r" % (seed,))
    every, draw_t = 0, None
    if independence is not None:
        try:
            every, draw_t = independence
        except (TypeError, ValueError):
            raise ValueError("independence is None or (every, draw_t)") from None
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or int(every) < 1 or not callable(draw_t):
            raise ValueError("independence is None or (every >= 1, a callable (n, t) -> (Yt, log_q_y))")
        if np.any(h == 0):
            raise ValueError("independence steps propose every column: no column may be frozen (step 0)")
    return dict(h=h, flags=flags, steps=int(steps), warmup=int(warmup), kernel=kernel, target=float(target),
                seed=None if seed is None else int(seed), every=int(every), draw_t=draw_t)


def check_chain_options(width, steps, warmup, record, least=2):
    """The `record` option of the Metropolis functions, checked with no device: None (nothing is recorded -> None), or a dict with
    the optional keys `levels` (the blocking levels, block lengths 1 ... 2^(levels - 1); None: min(8, floor(log2 T))) and `center`
    (one finite value per column, about which the deviations are taken; None: the starting points' means).  The states after the
    steps t >= warmup are recorded; T of them, an even count: of an odd number of post-warm-up states the FIRST is not recorded.
    ValueError for T < `least` (2 for the sums; `posterior_mcmc` asks for the 4 that split-R-hat needs) and for levels outside
    [1, min(16, floor(log2 T))].
    -> dict(T, first: the first recorded step, levels, center)."""
    if record is None:
        return None
    if not isinstance(record, dict) or set(record) - {"levels", "center"}:
        raise ValueError("record is None or a dict with the optional keys 'levels' and 'center', got %r" % (record,))
    count = int(steps) - int(warmup)
    T, first = count - (count & 1), int(warmup) + (count & 1)
    if T < max(int(least), 2):
        raise ValueError("at least %d recorded states are needed: steps - warmup = %d leaves %d" % (max(int(least), 2), count, max(T, 0)))
    top = min(16, T.bit_length() - 1)
    levels = record.get("levels")
    if levels is None:
        levels = min(CHAIN_DEFAULT_LEVELS, top)
    elif isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= top:
        raise ValueError("record['levels'] must be an integer in [1, min(16, floor(log2 T)) = %d] for T = %d recorded states, got %r"
                         % (top, T, levels))
    center = record.get("center")
    if center is not None:
        on_device = hasattr(center, "is_cuda") and center.is_cuda
        if tuple(center.shape if on_device else np.shape(center)) != (int(width),):
            raise ValueError("record['center'] must have one value per column (%d)" % width)
        if not on_device:
            center = np.asarray(center, dtype=np.float64)
            if not np.all(np.isfinite(center)):
                raise ValueError("record['center'] must be finite")
    return dict(T=T, first=first, levels=int(levels), center=center)


def blocking_tau(tau_levels, T: int, n: int) -> dict:
    """Which of the blocking estimates to quote.  tau_levels [levels] or [levels, columns]: the estimates of the integrated
    autocorrelation time at block lengths 1, 2, ..., 2^(levels - 1) (`nfisam_hip.chain_finish_t`'s "tau"), from n chains of T
    recorded states.  Level l has m_l = T >> l blocks per chain; it COUNTS when its pooled degrees of freedom n (m_l - 1) are at
    least BLOCKING_MIN_DOF = 64.
    -> dict(tau: the largest estimate among the levels that count (NaN where one of them is NaN: a column without spread);
    ess = n T / tau; resolved: True iff the longest block that counts is at least BLOCKING_PLATEAU = 4 times tau; level: the
    longest level that counts, -1 if none does -- then tau and ess are NaN and resolved is False).
    The blocking estimate grows with the block length towards the autocorrelation time and flattens once blocks are
    independent.  resolved = False therefore means that the plateau was NOT seen: tau is then a LOWER bound on the
    autocorrelation time and ess an UPPER bound on the effective sample size -- run longer, or record more levels."""
    tl = np.asarray(tau_levels, dtype=np.float64)
    if tl.ndim not in (1, 2) or tl.shape[0] < 1:
        raise ValueError("tau_levels must be [levels] or [levels, columns]")
    for name, v in (("T", T), ("n", n)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError("%s must be a positive integer, got %r" % (name, v))
    T, n = int(T), int(n)
    if T < 2 or T % 2 or tl.shape[0] > min(16, T.bit_length() - 1):
        raise ValueError("T must be even and >= 2, with at most min(16, floor(log2 T)) levels: got T = %d and %d levels"
                         % (T, tl.shape[0]))
    counts = n * ((T >> np.arange(tl.shape[0])) - 1) >= BLOCKING_MIN_DOF
    if not counts.any():
        nan = np.full(tl.shape[1:], np.nan)
        return dict(tau=nan, ess=nan.copy(), resolved=np.zeros(tl.shape[1:], dtype=bool), level=-1)
    top = int(np.flatnonzero(counts).max())                           # (the counts fall with the level: levels 0 ... top count)
    tau = np.max(tl[:top + 1], axis=0)                                # np.max keeps a NaN
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = n * T / tau
    return dict(tau=tau, ess=ess, resolved=float(1 << top) >= BLOCKING_PLATEAU * tau, level=top)


def chain_statistics_t(state, D, n, levels, T, center=None, wrap=None, tables=None) -> dict:
    """The statistics of the T states that `nfisam_hip.chain_record_t` folded into `state`: `nfisam_hip.chain_finish_t` on the
    device, then `blocking_tau` on the host.
    -> dict of numpy arrays: mean [D], within [D] (the pooled within-chain variance), rhat [D] (split-R-hat; NaN on a column
    without spread), tau_levels [levels, D], tau [D], ess [D], resolved [D] bool (False: tau is a lower bound, see
    `blocking_tau`); T, n, levels."""
    import nfisam_hip as _nh
    res = _nh.chain_finish_t(state, D, n, levels, T, center, wrap, tables=tables)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    pick = blocking_tau(host["tau"], int(T), int(n))
    return dict(mean=host["mean"], within=host["within"], rhat=host["rhat"], tau_levels=host["tau"], tau=pick["tau"],
                ess=pick["ess"], resolved=pick["resolved"], T=int(T), n=int(n), levels=int(levels))


def _lp64(v, n, what):
    import torch
    if not torch.is_tensor(v) or tuple(v.shape) != (n,):
        raise ValueError("%s must return a [n] = (%d,) device tensor" % (what, n))
    return v.to(torch.float64).contiguous()


def metropolis_refine_t(Xt, log_p_t, score_t, steps, step_size, circular=None, kernel="mala", warmup=0, target_accept=None,
                        seed=None, independence=None, after_step=None, log_q_t=None, record=None) -> dict:
    """n parallel Metropolis chains, one per column of the COLUMN-major device matrix Xt [D, n] (contiguous float32), IN PLACE
    and entirely on the device; their stationary distribution is exp(log p) itself.  log_p_t: a callable Xt -> log p [n]
    (float64 device tensor, e.g. around `nfisam_hip.factor_graph_log_density_t`); score_t: a callable Xt -> grad log p [D, n]
    (float64 column-major, e.g. around `nfisam_hip.factor_graph_score_t`; not called for kernel="rw").  A step proposes
    y = x + (h^2 / 2) grad log p + h z (kernel="mala") or y = x + h z ("rw") with `nfisam_hip.sample_propose_t`, evaluates
    log p (and the score) at y, and accepts or rejects every chain with `nfisam_hip.sample_accept_t`.  step_size: one step
    length or one per column, in the column's own unit (0 freezes the column: the chains sample the rest given it); circular
    [D]: columns that are angles.
    The first `warmup` steps scale ONE multiplier on h towards the acceptance rate `target_accept` (default 0.574 / 0.234):
    Robbins-Monro on log h, log m += (k + 1)^-0.6 (rate_k - target) with rate_k the fraction of chains that accepted step k,
    in torch ops on the device array -- no step waits for the host; a circular column's step stays at most WRAP_STEP_MAX.  After
    the warm-up h is fixed, which makes what follows a valid Markov chain.
    independence=(every, draw_t): every `every`-th step proposes Yt, log_q_y = draw_t(n, t) ([D, n] float32, [n]) -- fresh draws
    of a density q, e.g. the flow -- and accepts through the same entry with lp = log p - log q: a global jump between modes.
    It needs `log_q_t`, a callable Xt -> log q [n] for the current state.  after_step: a callable (Xt, step index).
    record: None, or dict(levels=None, center=None) (`check_chain_options`): the state after every step t >= warmup is folded
    into streaming accumulators on the device (`nfisam_hip.chain_record_t`, after the caller's own after_step), and the result
    gains `chains`, the dict of `chain_statistics_t`: per column the mean over chains and recorded states, split-R-hat, the
    blocking autocorrelation time tau, ess = n T / tau and `resolved` (False: tau is a lower bound).  An even number of states
    is recorded: of an odd number of post-warm-up steps the state after the FIRST is left out.  center None: the starting
    points' means (the circular mean of a circular column).  A frozen column (step 0) keeps its mean and within; its rhat, tau
    and ess are NaN and its resolved False.  Recording only reads Xt: the chains are the same bits with and without it, and
    with record=None not one key of the result changes.
    seed: the generator's key (None: one below 2^62 from numpy's global RNG, `DeviceSimulation`'s rule); step t uses counter
    word t, so two runs with one seed give the same bits.
    -> dict(accepts [n] int64: accepted local steps per chain; jump_accepts [n] int64; h [D] float64: the final step lengths;
    log_p [n] float64 (device tensors); steps, local_steps, jump_steps, warmup, seed).  steps = 0 leaves every bit alone.  Every
    option is checked before anything is launched."""
    import nfisam_hip as _nh
    import torch
    if not callable(log_p_t) or (kernel == "mala" and not callable(score_t)):
        raise ValueError("log_p_t (and, for kernel='mala', score_t) must be callables on Xt")
    if np.ndim(Xt) != 2:
        raise ValueError("Xt must be [columns, points]")
    opt = check_metropolis_options(int(Xt.shape[0]), steps, step_size, circular, kernel, warmup, target_accept, seed, independence)
    if opt["every"] and not callable(log_q_t):
        raise ValueError("independence steps need log_q_t, a callable Xt -> log q at the current state")
    if after_step is not None and not callable(after_step):
        raise ValueError("after_step must be a callable (Xt, step index)")
    rec = check_chain_options(int(Xt.shape[0]), opt["steps"], opt["warmup"], record)
    D, n = _nh._column_major_front("Xt", Xt)
    flags = opt["flags"]
    _nh.check_mcmc_args(D, n, opt["h"], flags.astype(np.uint8) if flags.any() else None)
    if rec is not None:
        _nh.check_chain_args(D, n, rec["levels"], rec["T"], 0, rec["center"], flags.astype(np.uint8) if flags.any() else None)
    seed = int(np.random.randint(0, 2 ** 62)) if opt["seed"] is None else opt["seed"]
    device, mala = Xt.device, kernel == "mala"
    zeros = torch.zeros(n, dtype=torch.int64, device=device)
    out = dict(accepts=zeros, jump_accepts=zeros.clone(), steps=opt["steps"], local_steps=0, jump_steps=0, warmup=opt["warmup"],
               seed=seed)
    with torch.cuda.device(device):
        tables = _nh.mcmc_tables(device, opt["h"], flags.astype(np.uint8) if flags.any() else None)
        h = tables["h"] = tables["h"].clone()                          # the loop's own array: the warm-up scales it in place
        lp = _lp64(log_p_t(Xt), n, "log_p_t").clone()
        if opt["steps"] == 0:
            return dict(out, h=h, log_p=lp)
        h0, log_m = h.clone(), torch.zeros((), dtype=torch.float64, device=device)
        cap = None if tables["wrap"] is None else \
            torch.full_like(h, float("inf")).masked_fill_(tables["wrap"] != 0, WRAP_STEP_MAX)
        Gx = score_t(Xt) if mala else None
        Yt = torch.empty_like(Xt)
        scratch = _nh.sample_accept_scratch(D, n, device)
        if rec is not None:
            center = rec["center"]
            if center is None:                                         # the starting points' means, as `posterior_summary` takes them
                circ = flags.astype(np.uint8) if flags.any() else None
                center = _nh.sample_moments_t(Xt, _nh.pack_moment_blocks(np.ones(D, dtype=np.int64)), np.arange(D), circ, None,
                                              checked=True)[0]
            chain_tb = _nh.chain_tables(device, center, flags.astype(np.uint8) if flags.any() else None)
            chain_st = _nh.chain_state(D, n, rec["levels"], device)
        for t in range(opt["steps"]):
            if opt["every"] and (t + 1) % opt["every"] == 0:           # a global jump: an independence proposal from q
                Y, lq_y = opt["draw_t"](n, t)
                wx = lp - _lp64(log_q_t(Xt), n, "log_q_t")
                lp_y = _lp64(log_p_t(Y), n, "log_p_t")
                wy = lp_y - _lp64(lq_y, n, "draw_t's log q")
                _, acc = _nh.sample_accept_t(Xt, Y, None, None, wx, wy, None, seed=seed, t=t, checked=True, tables=tables,
                                             scratch=scratch)
                lp = torch.where(acc != 0, lp_y, lp)
                if mala:
                    Gx = score_t(Xt)
                out["jump_accepts"] += acc
                out["jump_steps"] += 1
            else:
                _nh.sample_propose_t(Xt, Gx, None, seed=seed, t=t, Yt=Yt, checked=True, tables=tables)
                lp_y = _lp64(log_p_t(Yt), n, "log_p_t")
                Gy = score_t(Yt) if mala else None
                _, acc = _nh.sample_accept_t(Xt, Yt, Gx, Gy, lp, lp_y, None, seed=seed, t=t, checked=True, tables=tables,
                                             scratch=scratch)
                out["accepts"] += acc
                out["local_steps"] += 1
                if t < opt["warmup"]:
                    log_m += (out["local_steps"] ** -0.6) * (acc.to(torch.float64).mean() - opt["target"])
                    scaled = h0 * torch.exp(log_m)
                    h.copy_(scaled if cap is None else torch.minimum(scaled, cap))
            if after_step is not None:
                after_step(Xt, t)
            if rec is not None and t >= rec["first"]:
                _nh.chain_record_t(chain_st, Xt, t - rec["first"], rec["T"], rec["levels"], checked=True, tables=chain_tb)
        if rec is not None:
            out["chains"] = ch = chain_statistics_t(chain_st, D, n, rec["levels"], rec["T"], tables=chain_tb)
            frozen = opt["h"] == 0                                     # no spread within a chain: said by the step lengths, not left
            for k in ("rhat", "tau", "ess"):                           # to the rounding of a variance that is zero
                ch[k] = np.where(frozen, np.nan, ch[k])
            ch["tau_levels"] = np.where(frozen[None, :], np.nan, ch["tau_levels"])
            ch["resolved"] = ch["resolved"] & ~frozen
    return dict(out, h=h, log_p=lp)


def metropolis_refine(x, log_p, score, steps, step_size, circular=None, kernel="mala", warmup=0, target_accept=None, seed=None,
                      device=None, record=None) -> dict:
    """`metropolis_refine_t` for row-major points x [n, D] (numpy or torch) and a target given as callables on numpy:
    log_p(points [n, D] float64) -> [n], score(points) -> [n, D] (unused for kernel="rw").  The proposal and the accept step run
    on the device; the callables are called on the host once per step -- the convenience form.  record: as there.
    -> dict(x [n, D] float32 numpy: the chains' final states, log_p [n], accepts [n], h [D], steps, warmup, seed; with `record`
    also chains, the dict of `chain_statistics_t`)."""
    import nfisam_hip as _nh
    import torch
    if not callable(log_p) or (kernel == "mala" and not callable(score)):
        raise ValueError("log_p (and, for kernel='mala', score) must be callables points -> values")
    if np.ndim(x) != 2:
        raise ValueError("x must be [points, columns]")
    n, D = int(x.shape[0]), int(x.shape[1])
    if n < 1 or D < 1:
        raise ValueError("at least one point and one column are needed")
    opt = check_metropolis_options(D, steps, step_size, circular, kernel, warmup, target_accept, seed)
    check_chain_options(D, opt["steps"], opt["warmup"], record)
    device = _nh._row_major_front("metropolis_refine", device, x=x)
    Xt = _nh._columns(x, device)

    def host(Xt):
        return Xt.t().cpu().numpy().astype(np.float64)

    def log_p_t(Xt):
        v = np.asarray(log_p(host(Xt)), dtype=np.float64)
        if v.shape != (n,):
            raise ValueError("log_p must return [n] = (%d,), got %s" % (n, v.shape))
        return torch.from_numpy(v).to(Xt.device)

    def score_t(Xt):
        g = np.asarray(score(host(Xt)), dtype=np.float64)
        if g.shape != (n, D):
            raise ValueError("score must return the shape of x, %s, got %s" % ((n, D), g.shape))
        return torch.from_numpy(np.ascontiguousarray(g.T)).to(Xt.device)

    res = metropolis_refine_t(Xt, log_p_t, score_t, steps, step_size, circular, kernel, warmup, target_accept, seed, record=record)
    out = dict(x=Xt.t().cpu().numpy().copy(), log_p=res["log_p"].cpu().numpy(), accepts=res["accepts"].cpu().numpy(),
               h=res["h"].cpu().numpy(), steps=res["steps"], warmup=res["warmup"], seed=res["seed"])
    return dict(out, chains=res["chains"]) if record is not None else out


# ---- curvature: matrix-free conjugate gradients on Hessian-vector products, truncated Newton ascent (nfisam_factor_graph_hvp) ----
NEWTON_GTOL, NEWTON_BACKTRACKS = 1e-3, 10


def check_newton_options(width, steps=0, cg_iters=None, rtol=1e-8, damping=0.0, gtol=NEWTON_GTOL, backtracks=NEWTON_BACKTRACKS,
                         scale=None, circular=None):
    """Every option of `conjugate_gradient_t` / `newton_refine_t`, checked with no device: steps an integer >= 0; cg_iters an
    integer >= 1 (None: width, the exact solve of a quadratic); rtol in (0, 1); damping one finite value >= 0 or one per
    column; gtol positive and finite; backtracks an integer in 0..60; scale one finite value >= 0 per column (None: ones; 0: a
    column that does not count in the gradient norm); circular one flag per column.
    -> dict(steps, cg_iters, rtol, damping [width], gtol, backtracks, scale [width], flags [width])."""
    def whole(name, v, lo, hi=None):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
            raise ValueError("%s must be an integer %s, got %r" % (name, ">= %d" % lo if hi is None else "in %d..%d" % (lo, hi), v))
        return int(v)
    width = whole("width", width, 1)
    steps = whole("steps", steps, 0)
    cg_iters = width if cg_iters is None else whole("cg_iters", cg_iters, 1)
    backtracks = whole("backtracks", backtracks, 0, 60)
    if np.ndim(rtol) != 0 or not (np.isfinite(rtol) and 0.0 < rtol < 1.0):
        raise ValueError("rtol must lie in (0, 1), got %r" % (rtol,))
    if np.ndim(gtol) != 0 or not (np.isfinite(gtol) and gtol > 0.0):
        raise ValueError("gtol must be positive and finite, got %r" % (gtol,))
    damp = np.asarray(0.0 if damping is None else damping, dtype=np.float64).reshape(-1)
    damp = np.broadcast_to(damp, (width,)).copy() if damp.size == 1 else damp
    if damp.size != width or not np.all(np.isfinite(damp) & (damp >= 0)):
        raise ValueError("damping is one finite value >= 0, or one per column (%d)" % width)
    sc = np.ones(width) if scale is None else np.asarray(scale, dtype=np.float64).reshape(-1)
    if sc.size != width or not np.all(np.isfinite(sc) & (sc >= 0)):
        raise ValueError("scale: one finite value >= 0 per column (%d)" % width)
    return dict(steps=steps, cg_iters=cg_iters, rtol=float(rtol), damping=damp, gtol=float(gtol), backtracks=backtracks, scale=sc,
                flags=_column_flags(circular, width))


def conjugate_gradient_t(hvp, Bt, iters, rtol, damping=None, precond=None):
    """Solves (-H_p + diag(damping)) d_p = b_p for every column p of Bt [D, n] (float64 tensor) at once by conjugate
    gradients with per-point scalars, never forming a matrix: `hvp(Vt)` returns Ht with Ht[:, p] = H_p Vt[:, p] (float64, the
    layout of `nfisam_hip.factor_graph_hvp_t`, which is the hot path; the vector work is torch float64 where Bt lies).  H is the
    Hessian of a log density: at a mode -H is positive definite.  damping: None, one value or one per row of Bt.
    A point stops when its residual is <= rtol |b|, after `iters` products, or when it meets a direction p with
    p'(-H + damping) p <= 0 (or not a number): it then keeps what it has (Steihaug's rule), b itself on the first iteration.
    A stopped point's columns are frozen by masks: the batch keeps its shape, so the others' bits are those of a run without it.
    precond: None, or a positive float64 tensor [D, n] (or [D, 1]) M^-1, the inverse of a diagonal that resembles -H + damping
    (`hessian_diagonal_t`): the iteration is then the preconditioned one -- a SLAM Hessian holds 1 / sigma^2 of millimetres
    next to 1 / sigma^2 of metres, and without its diagonal scaled out conjugate gradients do not arrive within D products.
    The stopping rule stays the plain residual's, and a first-iteration refusal keeps M^-1 b.
    -> dict(x [D, n], residual [n]: |r| / |b| of the iterate by the recurrence (0 for b = 0; a point that kept b itself reports
    1), iters [n] int64: products used, negative_curvature [n] bool)."""
    import torch
    if not torch.is_tensor(Bt) or Bt.ndim != 2 or Bt.dtype != torch.float64:
        raise ValueError("Bt must be a float64 [columns, points] tensor")
    D, n = int(Bt.shape[0]), int(Bt.shape[1])
    opt = check_newton_options(max(D, 1), cg_iters=iters, rtol=rtol, damping=damping)
    damp = torch.from_numpy(opt["damping"]).to(Bt.device).unsqueeze(1) if opt["damping"].any() else None
    if precond is not None and not (torch.is_tensor(precond) and precond.dtype == torch.float64 and precond.ndim == 2
                                    and tuple(precond.shape) in ((D, n), (D, 1))):
        raise ValueError("precond must be a float64 [columns, points] or [columns, 1] tensor")
    X, Rt = torch.zeros_like(Bt), Bt.clone()
    P = Bt.clone() if precond is None else precond * Bt
    bnorm = torch.linalg.vector_norm(Bt, dim=0)
    rs = (Rt * P).sum(0)                                              # r'z, z = M^-1 r (r'r without a preconditioner)
    active = bnorm > 0
    used = torch.zeros(n, dtype=torch.int64, device=Bt.device)
    neg = torch.zeros(n, dtype=torch.bool, device=Bt.device)
    for k in range(opt["cg_iters"]):
        if not bool(active.any()):
            break
        AP = -hvp(P)
        if damp is not None:
            AP = AP + damp * P
        pAp = (P * AP).sum(0)
        bad = active & ~(pAp > 0)
        if k == 0:
            X = torch.where(bad.unsqueeze(0), P, X)
        neg |= bad
        active = active & ~bad
        used += active
        alpha = torch.where(active, rs / pAp, torch.zeros_like(rs))
        X = torch.where(active.unsqueeze(0), X + alpha * P, X)
        Rt = torch.where(active.unsqueeze(0), Rt - alpha * AP, Rt)
        Z = Rt if precond is None else precond * Rt
        rs_new = (Rt * Z).sum(0)
        go = active & ~(torch.linalg.vector_norm(Rt, dim=0) <= opt["rtol"] * bnorm)
        P = torch.where(go.unsqueeze(0), Z + (rs_new / rs) * P, P)
        rs = torch.where(active, rs_new, rs)
        active = go
    ratio = torch.where(bnorm > 0, torch.linalg.vector_norm(Rt, dim=0) / bnorm, torch.zeros_like(bnorm))
    return dict(x=X, residual=ratio, iters=used, negative_curvature=neg)


def probe_colours(row_groups, width):
    """Column classes for probing a sparse symmetric matrix's diagonal: `row_groups` lists, per factor, the columns the factor
    couples (every pair inside a group may hold an entry); two columns share a class only if no group holds both, so a product
    with a class's indicator vector shows H_cc alone in the rows c of that class.  Greedy, columns in ascending order.
    -> list of int64 arrays that partition range(width).  No device."""
    near = [set() for _ in range(width)]
    for g in row_groups:
        g = [int(c) for c in g]
        if g and (min(g) < 0 or max(g) >= width):
            raise ValueError("a group names a column outside the %d columns" % width)
        for c in g:
            near[c].update(g)
    colour = np.full(width, -1, dtype=np.int64)
    for c in range(width):
        taken = {int(colour[o]) for o in near[c] if colour[o] >= 0}
        k = 0
        while k in taken:
            k += 1
        colour[c] = k
    return [np.flatnonzero(colour == k) for k in range(int(colour.max()) + 1 if width else 0)]


def hessian_diagonal_t(hvp, colours, width, n, device):
    """diag(H_p) for every point p, [width, n] float64 on `device`, from len(colours) Hessian-vector products: one per class of
    `probe_colours`, along the class's indicator vector."""
    import torch
    diag = torch.zeros(width, n, dtype=torch.float64, device=device)
    for cols in colours:
        idx = torch.as_tensor(cols, device=device)
        V = torch.zeros(width, n, dtype=torch.float64, device=device)
        V[idx] = 1.0
        diag[idx] = hvp(V)[idx]
    return diag


def inverse_diagonal(diag_h, damp):
    """M^-1 for `conjugate_gradient_t` from diag(H): 1 / (-H_cc + damping_c) where that is positive, else 1 (a column
    without curvature of the right sign is left unscaled)."""
    import torch
    m = -diag_h if damp is None else -diag_h + damp
    return torch.where(m > 0, 1.0 / torch.where(m > 0, m, torch.ones_like(m)), torch.ones_like(m))


def _wrapped_step(Xt, Dt, s, flags_t):
    """float32(x + s d) with the heading rows brought into [-pi, pi) the way `nfisam_hip.sample_step_t` does it."""
    import torch
    y = Xt.to(torch.float64) + s * Dt
    f = y.to(torch.float32)
    if flags_t is not None:
        w = (torch.remainder(y + np.pi, 2.0 * np.pi) - np.pi).to(torch.float32)
        inside = (w.to(torch.float64) < np.pi) & (w.to(torch.float64) >= -np.pi)
        w = torch.where(inside | torch.isnan(y), w, torch.full_like(w, -3.1415925))      # +-float32(pi) lies outside
        f = torch.where(flags_t, w, f)
    return f


def newton_refine_t(Xt, score_hvp, log_p, steps, cg_iters=None, rtol=1e-8, damping=0.0, gtol=NEWTON_GTOL,
                    backtracks=NEWTON_BACKTRACKS, scale=None, circular=None, colours=None) -> dict:
    """Truncated-Newton ascent of log p for every point of the COLUMN-major matrix Xt [D, n] (contiguous float32) at once, IN
    PLACE, each point alone.  `score_hvp(Xt, Vt)` -> (Ht, Gt): the Hessian-vector products along Vt [D, n] float64 and the
    score at Xt from one pass (`nfisam_hip.factor_graph_hvp_t(..., score=True)`); `log_p(Xt)` -> [n] float64.
    A step: ONE `score_hvp` call with a zero direction gives g; `conjugate_gradient_t` solves (-H + diag(damping)) d = g with
    at most `cg_iters` (None: D) further products; then the step length backtracks from 1 by halving, at most `backtracks`
    times, every trial one `log_p` launch: the first trial with log p above the point's present value is taken, into the
    float32 point, headings (`circular` [D]) wrapped as `sample_step_t` wraps them.  A point whose trials all fail stays, so a
    point never falls and its present position is its best iterate.  colours: the classes of `probe_colours` for H's
    sparsity; with them every step first reads diag(H) at the points (one product per class) and the conjugate gradients are
    preconditioned with it.  A step is 1 + (classes) + (products) + (trials) launches, at most 2 + classes + cg_iters +
    backtracks.  A point is converged when the scaled infinity norm of its score, max_c |g_c| / scale_c (scale
    [D]: 1 / spread standardises, as in `stein_variational_refine_t`; 0 leaves a column out; None: ones), is <= gtol; converged
    points take no further steps, and the loop ends when every point is.
    The float32 floor the defaults are chosen from: next to a mode the score at a float32 point is about |H| times half the
    float32 spacing of the coordinate.  In standardised units (|H| spread^2 about (spread / sigma)^2, about 1 when the points
    are spread like the mode is wide) that is spacing / (2 sigma): 3.8e-4 for a coordinate of 100 m (spacing 2^-17 m) and a mode
    1 cm wide.  gtol = 1e-3 is the next power of ten above it -- below the floor `converged` could never be reported.  A
    Newton step is at most about one spread; a spread of 1 cm is 2^10.4 spacings at 100 m, so the 11th halving moves such a
    coordinate by less than its spacing: backtracks = 10.
    -> dict(log_p [n] float64 at the final points, start_log_p [n], grad_norm [n] (at the final points), converged [n] bool,
    negative_curvature [n] bool (met by the CG of the last step a point took), steps: steps taken).  steps = 0 leaves every
    bit alone.  Every option is checked (`check_newton_options`) before anything is launched."""
    import torch
    if not callable(score_hvp) or not callable(log_p):
        raise ValueError("score_hvp and log_p must be callables")
    if not torch.is_tensor(Xt) or Xt.ndim != 2 or Xt.dtype != torch.float32 or not Xt.is_contiguous():
        raise ValueError("Xt must be a contiguous float32 [columns, points] tensor")
    D, n = int(Xt.shape[0]), int(Xt.shape[1])
    if D < 1 or n < 1:
        raise ValueError("newton_refine: no points")
    opt = check_newton_options(D, steps, cg_iters, rtol, damping, gtol, backtracks, scale, circular)
    dev = Xt.device
    inv_scale = torch.from_numpy(np.where(opt["scale"] > 0, 1.0 / np.where(opt["scale"] > 0, opt["scale"], 1.0), 0.0)).to(dev).unsqueeze(1)
    flags_t = torch.from_numpy(opt["flags"]).to(dev).unsqueeze(1) if opt["flags"].any() else None
    zero = torch.zeros(D, n, dtype=torch.float64, device=dev)
    damp_t = torch.from_numpy(opt["damping"]).to(dev).unsqueeze(1) if opt["damping"].any() else None

    def gradient():
        Gt = score_hvp(Xt, zero)[1]
        return Gt, (Gt.abs() * inv_scale).amax(0)

    lp = log_p(Xt).clone()
    start = lp.clone()
    neg = torch.zeros(n, dtype=torch.bool, device=dev)
    taken = 0
    Gt, gnorm = gradient()
    for t in range(opt["steps"]):
        moving = ~(gnorm <= opt["gtol"])
        if not bool(moving.any()):
            break
        hvp = lambda Vt: score_hvp(Xt, Vt)[0]
        minv = None if colours is None else inverse_diagonal(hessian_diagonal_t(hvp, colours, D, n, dev), damp_t)
        cg = conjugate_gradient_t(hvp, torch.where(moving.unsqueeze(0), Gt, zero), opt["cg_iters"], opt["rtol"], opt["damping"],
                                  precond=minv)
        neg = torch.where(moving, cg["negative_curvature"], neg)
        pending, s = moving.clone(), 1.0
        for b in range(opt["backtracks"] + 1):
            trial = torch.where(pending.unsqueeze(0), _wrapped_step(Xt, cg["x"], s, flags_t), Xt)
            lp_t = log_p(trial)
            ok = pending & (lp_t > lp)
            Xt.copy_(torch.where(ok.unsqueeze(0), trial, Xt))
            lp = torch.where(ok, lp_t, lp)
            pending = pending & ~ok
            if not bool(pending.any()):
                break
            s *= 0.5
        taken += 1
        Gt, gnorm = gradient()
    return dict(log_p=lp, start_log_p=start, grad_norm=gnorm, converged=gnorm <= opt["gtol"], negative_curvature=neg, steps=taken)

