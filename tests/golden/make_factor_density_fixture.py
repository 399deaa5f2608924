#!/usr/bin/env python3
"""Factor densities from the REFERENCE ITSELF (runs only where the reference checkout is present, `make_pipeline_fixture.REF`; nothing of it travels).

Writes tests/golden/factor_density.npz, the yardstick of `Factors.*.log_pdf` and of the device entry
`nfisam_factor_graph_log_density`:

 (a) per factor type, hand-chosen and random cases: the constructor parameters, float32 points, and the reference's
     `log_pdf` at those points in float64.  The points are rounded to float32 BEFORE the reference sees them: the device
     works on float32 sample matrices and the contract is the float64 formula at the float32 point.  Covered on purpose:
     heading residuals inside and outside the |theta| < 1e-5 branch of the log-map Jacobian, headings either side of +-pi,
     a range of exactly 0, mixtures of 2 / 3 / 4 candidates, a null-hypothesis factor.
 (b) the whole graphs tests/data/ManhattanPlaza136 (272 factors) and tests/data/Plaza1ADA0.4EFG (1584 factors), read with
     the reference's `graph_file_parser(..., prior_cov_scale=0.1)`: 16 (Manhattan) / 6 (Plaza1-ADA) points per s in {0.003, 0.03, 0.3}, each the ground
     truth + N(0, s^2) per coordinate; per-factor `log_pdf` terms and the `JointFactor.log_pdf` total
     (src/sampler/sampler_utils.py:85-98).

Where the numbers come from:
  * the SE(2), range and mixture classes: the reference's own `log_pdf` bodies (src/factors/Factors.py:823-827, :1443-1448,
    :2724-2730, :2195-2201, :3126-3133);
  * the Gaussian normaliser and quadratic form inside them come from `TransportMaps.Distributions.GaussianDistribution`,
    which is absent here: `make_pipeline_fixture.write_stubs` restates it (multivariate normal by precision matrix).  That
    restatement is ours, not the reference's; tests/test_factor_density_cpu.py checks the normaliser independently with a
    closed-form multivariate normal;
  * R2RelativeGaussianLikelihoodFactor: its `log_pdf` goes through a TransportMaps likelihood (stubbed out), so the rows
    are evaluated with its own `evaluate_loglike` (:1070-1074), point by point;
  * UnaryR2RangeGaussianPriorFactor (the later of its two definitions, :2226): it has no usable density -- its
    distribution defines no log_pdf and `evaluate_loglike` (:2301-2303) subtracts mu inside the norm.  The stored value is
    the reference's R2RangeGaussianLikelihoodFactor.log_pdf with the first end pinned at the centre: the density of the
    radius its sampler draws.

No term may be non-finite: the script stops if one is (change the points, never mask a comparison).

    python tests/golden/make_factor_density_fixture.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_pipeline_fixture import REF, write_stubs  # noqa: E402

OUT = os.path.join(HERE, "factor_density.npz")
DATA = os.path.join(os.path.dirname(HERE), "data")
GRAPHS = {"manhattan136": "ManhattanPlaza136", "plaza1ada": "Plaza1ADA0.4EFG"}
SCALES = (0.003, 0.03, 0.3)
# points per scale: 48 points of Manhattan-136, 18 of Plaza1-ADA (its 1584 x 2342 graph at 48 points would put the file past
# the size limit of a committed file; float64 terms of random points do not compress)
POINTS_PER_SCALE = {"manhattan136": 16, "plaza1ada": 6}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def spd(rng, d, lo, hi):
    """Random covariance with eigenvalues log-uniform in [lo, hi]."""
    q, _ = np.linalg.qr(rng.randn(d, d))
    return (q * np.exp(rng.uniform(np.log(lo), np.log(hi), d))) @ q.T


def main():
    tmp = tempfile.mkdtemp(prefix="nfisam_ref_")
    write_stubs(os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(REF, "src"))
    sys.dont_write_bytecode = True
    import matplotlib
    matplotlib.use("Agg")
    import factors.Factors as F
    from geometry.TwoDimension import SE2Pose
    from sampler.sampler_utils import JointFactor
    from slam.RunBatch import graph_file_parser
    from slam.Variables import R2Variable, SE2Variable, VariableType

    rng = np.random.RandomState(20261016)
    out, cases = {}, []
    X, Y = SE2Variable("X0"), SE2Variable("X1")
    L = [R2Variable("L%d" % i, variable_type=VariableType.Landmark) for i in range(4)]

    def add(cls, params, x, ref):
        ref = np.asarray(ref, dtype=np.float64).reshape(-1)
        assert ref.shape[0] == x.shape[0] and np.all(np.isfinite(ref)), (cls, ref)
        i = len(cases)
        cases.append(cls)
        out["a%03d_params" % i] = np.asarray(params, dtype=np.float64)
        out["a%03d_x" % i] = x.astype(np.float32)
        out["a%03d_ref" % i] = ref

    def heading_rows(base_theta, n):
        """Heading residuals against `base_theta`: 0, inside / at / outside the 1e-5 branch, large, and across +-pi."""
        res = np.concatenate([[0.0, 3e-7, -8e-6, 9.9e-6, 1.01e-5, -2e-5, 1e-3, -0.4, 2.9, -3.1, 3.14, -3.14],
                              rng.uniform(-np.pi, np.pi, n)])
        return base_theta + res

    # ---- SE(2) prior: params = pose(3) + covariance(9) -----------------------------------------------------------------
    for pose, cov in [((0.0, 0.0, 0.0), np.diag([1e-8, 1e-10, 1e-12])),             # the Plaza first-pose prior
                      ((1.5, -2.0, 3.1), np.diag([1e-4, 1e-6, 1e-8])),               # Manhattan-136's, heading next to +pi
                      ((-40.0, 25.0, -3.13), spd(rng, 3, 1e-3, 1e-1)),
                      ((3.0, 4.0, 0.7), spd(rng, 3, 1e-2, 1.0))]:
        th = heading_rows(pose[2], 20)
        scale = np.sqrt(np.diag(cov))
        x = np.stack([pose[0] + 3 * scale[0] * rng.randn(th.size), pose[1] + 3 * scale[1] * rng.randn(th.size), th], 1)
        if cov[2, 2] < 1e-6:                                        # a tight heading: keep the term's magnitude plausible
            x[12:, 2] = pose[2] + 4 * scale[2] * rng.randn(th.size - 12)
        x[-4:, 2] += 2 * np.pi * np.array([1, -1, 2, -2])           # the same headings, other representatives
        x = f32(x)
        f = F.UnarySE2ApproximateGaussianPriorFactor(var=X, prior_pose=SE2Pose(*pose), covariance=cov)
        add("UnarySE2ApproximateGaussianPriorFactor", list(pose) + list(cov.ravel()), x, f.log_pdf(x))

    # ---- SE(2) relative pose: params = observation(3) + covariance(9) ---------------------------------------------------
    for obs, cov in [((1.0, 0.0, 0.0), np.diag([1e-4, 1e-4, 1e-4])),
                     ((2.0, 0.1, np.pi / 2), np.diag([1e-3, 1e-3, 1e-4])),
                     ((0.5, -0.3, 3.0), spd(rng, 3, 1e-4, 1e-2)),
                     ((-1.0, 2.0, -2.5), spd(rng, 3, 1e-2, 1.0))]:
        n = 32
        xi = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-np.pi, np.pi, n)], 1)
        xi[:6, 2] = [3.14, -3.14, 3.1415, -3.1415, 0.0, 1.0]
        xi = f32(xi)
        th = heading_rows(0.0, n - 12)
        sc = np.sqrt(np.diag(cov))
        rel = np.stack([obs[0] + 3 * sc[0] * rng.randn(n), obs[1] + 3 * sc[1] * rng.randn(n), obs[2] + th], 1)
        c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
        xj = np.stack([xi[:, 0] + c * rel[:, 0] - s * rel[:, 1], xi[:, 1] + s * rel[:, 0] + c * rel[:, 1],
                       xi[:, 2] + rel[:, 2]], 1)
        xj[::2, 2] = (xj[::2, 2] + np.pi) % (2 * np.pi) - np.pi     # half wrapped, half left past +-pi
        x = f32(np.concatenate([xi, xj], 1))
        f = F.SE2RelativeGaussianLikelihoodFactor(var1=X, var2=Y, observation=SE2Pose(*obs), covariance=cov)
        add("SE2RelativeGaussianLikelihoodFactor", list(obs) + list(cov.ravel()), x, f.log_pdf(x))

    # ---- ranges: params = observation, sigma ------------------------------------------------------------------------------
    def range_points(d1, d2, n, d, sigma):
        a = rng.uniform(-30, 30, (n, d1))
        b = rng.uniform(-30, 30, (n, d2))
        phi = rng.uniform(-np.pi, np.pi, n)
        r = d + sigma * rng.randn(n) * np.where(np.arange(n) % 3 == 0, 5.0, 1.0)
        b[:, 0], b[:, 1] = a[:, 0] + r * np.cos(phi), a[:, 1] + r * np.sin(phi)
        b[0, :2] = a[0, :2]                                            # a range of exactly 0
        return f32(np.concatenate([a, b], 1))

    for d, sigma in [(5.0, 0.5), (0.3, 0.4), (37.25, 2.0), (12.0, 0.05)]:
        x = range_points(3, 2, 24, d, sigma)
        f = F.SE2R2RangeGaussianLikelihoodFactor(var1=X, var2=L[0], observation=d, sigma=sigma)
        add("SE2R2RangeGaussianLikelihoodFactor", [d, sigma], x, f.log_pdf(x))
        x = range_points(2, 2, 24, d, sigma)
        f = F.R2RangeGaussianLikelihoodFactor(var1=L[0], var2=L[1], observation=d, sigma=sigma)
        add("R2RangeGaussianLikelihoodFactor", [d, sigma], x, f.log_pdf(x))

    # ---- ambiguous data association: params = k, weights(k), observation, sigma; x = [X | L0 .. L(k-1)] ---------------------
    for k, d, sigma in [(2, 6.0, 0.5), (3, 11.0, 1.0), (4, 4.0, 0.4), (4, 20.0, 2.0)]:
        w = rng.uniform(0.2, 1.0, k)
        w /= w.sum()
        n = 32
        pose = np.stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.uniform(-np.pi, np.pi, n)], 1)
        lm = rng.uniform(-15, 15, (n, 2 * k))
        for i in range(n):                                             # every row near (within a few sigma of) one hypothesis
            j = i % k
            phi, r = rng.uniform(-np.pi, np.pi), d + sigma * rng.randn() * (1.0 + 4.0 * (i % 5 == 0))
            lm[i, 2 * j:2 * j + 2] = pose[i, :2] + r * np.array([np.cos(phi), np.sin(phi)])
        x = f32(np.concatenate([pose, lm], 1))
        f = F.AmbiguousDataAssociationFactor(observer_var=X, observed_vars=L[:k], weights=w,
                                             binary_factor_class=F.SE2R2RangeGaussianLikelihoodFactor, observation=d,
                                             sigma=sigma)
        add("AmbiguousDataAssociationFactor", [k] + list(w) + [d, sigma], x, f.log_pdf(x))

    # ---- null hypothesis: params = weights(2), observation, sigma, null_sigma_scale; x = [X | L0] -----------------------------
    for w, d, sigma, scale in [((0.9, 0.1), 8.0, 0.5, 10.0), ((0.5, 0.5), 3.0, 0.2, 4.0)]:
        x = range_points(3, 2, 32, d, sigma * np.sqrt(scale))
        f = F.BinaryFactorWithNullHypo(var1=X, var2=L[0], weights=np.array(w),
                                       binary_factor_class=F.SE2R2RangeGaussianLikelihoodFactor, observation=d, sigma=sigma,
                                       null_sigma_scale=scale)
        add("BinaryFactorWithNullHypo", list(w) + [d, sigma, scale], x, f.log_pdf(x))

    # ---- R2 Gaussian prior: params = mu(2), covariance(4) ------------------------------------------------------------------------
    for mu, cov in [((0.0, 0.0), np.diag([1e-4, 1e-4])), ((12.5, -7.0), spd(rng, 2, 1e-2, 4.0))]:
        x = f32(np.array(mu) + rng.randn(24, 2) @ np.linalg.cholesky(cov).T * 2.0)
        f = F.UnaryR2GaussianPriorFactor(var=L[0], mu=np.array(mu), covariance=cov)
        add("UnaryR2GaussianPriorFactor", list(mu) + list(cov.ravel()), x, f.log_pdf(x))

    # ---- R2 relative: params = observation(2), covariance(4); rows through evaluate_loglike ------------------------------
    for obs, cov in [((1.0, 2.0), np.diag([1e-2, 1e-2])), ((-3.5, 0.25), spd(rng, 2, 1e-3, 1.0))]:
        a = rng.uniform(-20, 20, (24, 2))
        b = a + np.array(obs) + rng.randn(24, 2) @ np.linalg.cholesky(cov).T * 2.0
        x = f32(np.concatenate([a, b], 1))
        f = F.R2RelativeGaussianLikelihoodFactor(var1=L[0], var2=L[1], observation=np.array(obs), covariance=cov)
        add("R2RelativeGaussianLikelihoodFactor", list(obs) + list(cov.ravel()), x, [f.evaluate_loglike(r) for r in x])

    # ---- R2 range prior: params = center(2), mu, sigma; the reference's range likelihood with one end at the centre ----
    for center, mu, sigma in [((0.0, 0.0), 5.0, 0.5), ((10.0, -4.0), 1.0, 2.0)]:
        x = range_points(2, 2, 24, mu, sigma)
        x[:, :2] = f32(np.array(center))
        x = f32(x)
        x[0, 2:] = x[0, :2]
        f = F.R2RangeGaussianLikelihoodFactor(var1=L[0], var2=L[1], observation=mu, sigma=sigma)
        add("UnaryR2RangeGaussianPriorFactor", list(center) + [mu, sigma], x[:, 2:], f.log_pdf(x))
    out["a_classes"] = np.array(cases)

    # ---- (b) whole graphs --------------------------------------------------------------------------------------------------
    for key, folder in GRAPHS.items():
        nodes, truth, factors = graph_file_parser(data_file=os.path.join(DATA, folder, "factor_graph.fg"), data_format="fg",
                                                  prior_cov_scale=0.1)
        joint = JointFactor(factors, nodes)
        t = np.concatenate([np.asarray(truth[v], dtype=np.float64).ravel() for v in nodes])
        pts = np.concatenate([t + s * rng.randn(POINTS_PER_SCALE[key], t.size) for s in SCALES])
        x = pts.astype(np.float32)
        x64 = x.astype(np.float64)
        terms = np.stack([np.asarray(f.log_pdf(x64[:, joint._factor_to_indices[f]]), dtype=np.float64).reshape(-1)
                          for f in factors])
        total = np.asarray(joint.log_pdf(x64), dtype=np.float64).reshape(-1)
        assert np.all(np.isfinite(terms)) and np.all(np.isfinite(total)), "non-finite reference value: change the points"
        out[key + "_vars"] = np.array([str(v.name) for v in nodes])
        out[key + "_dims"] = np.array([v.dim for v in nodes], dtype=np.int32)
        out[key + "_factors"] = np.array([f.__class__.__name__ + " " + " ".join(str(v.name) for v in f.vars) for f in factors])
        out[key + "_scale"] = np.repeat(np.array(SCALES), POINTS_PER_SCALE[key])
        out[key + "_x"] = x
        out[key + "_terms"] = terms
        out[key + "_total"] = total
        print(key, len(factors), "factors", x.shape, "total range", total.min(), total.max())
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
