"""Writes tests/golden/sample_density.npz: what scipy.stats.gaussian_kde (scipy 1.15) says about three small float32 sample
sets, for tests/test_sample_density_cpu.py and tests/test_sample_density_gpu.py -- neither of which imports scipy.

    python tests/golden/make_sample_density_fixture.py

Per case k = 0, 1, 2 with (d, n, m) = (1, 70, 130), (2, 130, 70), (3, 200, 65): x{k} [n, d] float32 samples (correlated columns,
offset by tens of metres), q{k} [m, d] float32 queries (most among the samples, some in the tails, four thousands of
bandwidths away), w{k} [n] float64 weights (case 1 only; one of them zero), and per rule in ("scott", "silverman")
logpdf_{rule}{k} [m] = gaussian_kde(x.T, bw_method=rule, weights=w).logpdf(q.T), cov_{rule}{k} [d, d] = its `covariance`
(the bandwidth matrix), and neff{k}.
bimodal [500] float32: half N(-5, 0.3^2), half N(5, 0.3^2), the set on which Scott's rule is several times too wide."""
import os

import numpy as np
from scipy.stats import gaussian_kde

CASES = [(1, 70, 130), (2, 130, 70), (3, 200, 65)]
OFFSET = np.array([37.5, -62.25, 18.0])


def case(k, d, n, m):
    rng = np.random.default_rng(100 + k)
    A = np.tril(rng.normal(size=(d, d))) + 1.5 * np.eye(d)         # correlated columns
    x = (rng.normal(size=(n, d)) @ A.T + OFFSET[:d]).astype(np.float32)
    q = rng.normal(size=(m, d)) @ A.T * 1.5 + OFFSET[:d]
    q[-8:-4] += 25.0 * rng.normal(size=(4, d))                     # the tails
    q[-4:] += 3000.0 * np.sign(rng.normal(size=(4, d)))            # thousands of bandwidths away
    q = q.astype(np.float32)
    q[0] = x[0]                                                    # a query on a sample
    w = None
    if k == 1:
        w = rng.uniform(0.2, 3.0, size=n)
        w[7] = 0.0
    out = {"x%d" % k: x, "q%d" % k: q}
    if w is not None:
        out["w%d" % k] = w
    for rule in ("scott", "silverman"):
        kde = gaussian_kde(x.T.astype(np.float64), bw_method=rule, weights=w)
        out["logpdf_%s%d" % (rule, k)] = kde.logpdf(q.T.astype(np.float64))
        out["cov_%s%d" % (rule, k)] = np.atleast_2d(kde.covariance)
        out["neff%d" % k] = np.float64(kde.neff)
    return out


def bimodal():
    rng = np.random.default_rng(7)
    return np.concatenate([rng.normal(-5.0, 0.3, 250), rng.normal(5.0, 0.3, 250)]).astype(np.float32)


if __name__ == "__main__":
    data = {"bimodal": bimodal()}
    for k, (d, n, m) in enumerate(CASES):
        data.update(case(k, d, n, m))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sample_density.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    for key in sorted(data):
        print(key, np.shape(data[key]), data[key].dtype)
