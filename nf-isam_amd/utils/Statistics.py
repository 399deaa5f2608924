"""utils.Statistics — maximum mean discrepancy used as the posterior parity metric
(reference: src/utils/Statistics.py:13-84; the biased estimator `MMDb` with an RBF kernel of
bandwidth sigma is what the reference's evaluation scripts report,
example/slam/small_range_gaussian_problem/icra_paper/mmd_rmse_time_da_plot_grid.py:167,245)."""
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
    if sigma is None:
        sig = np.ones(len(pairs)) if estimator == "mmd" else np.sqrt(dims.astype(np.float64))
    else:
        sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (len(pairs),)) if np.ndim(sigma) == 0 else \
            np.asarray(sigma, dtype=np.float64).reshape(-1)
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
    table = _nh.pack_mmd_blocks(dims, sig)
    sums = _nh.mmd_sums(x, y, table, xcols, ycols, scale=sc, wrap=wr, device=device)
    return mmd_from_sums(sums.cpu().numpy(), m, n, estimator)
