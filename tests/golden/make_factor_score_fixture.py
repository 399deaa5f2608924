#!/usr/bin/env python3
"""Factor scores and a kernel Stein discrepancy from the REFERENCE ITSELF (runs only where the reference checkout is present,
`make_pipeline_fixture.REF`; nothing of it travels).  Only data is written.

Writes tests/golden/factor_score.npz, the yardstick of `Factors.*.grad_x_log_pdf`, of the device entries
`nfisam_factor_graph_score` / `nfisam_sample_ksd` and of `Statistics.Gaussian_kernel_stein_discrepancy`:

 (a) per factor type: every part-(a) case of factor_density.npz (the same constructor parameters, the same float32 points,
     which are NOT stored again).  a%03d_ref [n, width] float64 is
       * the reference's own `grad_x_log_pdf` for the SE(2) prior and relative pose, the two range likelihoods and the mixtures
         (src/factors/Factors.py:829-850, :1450-1478, :2732-2751, :2203-2223, :3135-3143);
       * Richardson central differences, (4 D(h) - D(2h)) / 3 with h = 1e-3 of the factor's sigma per coordinate, of the value
         source make_factor_density_fixture.py documents, for the three R2 classes whose density goes through the stubbed
         TransportMaps: UnaryR2GaussianPriorFactor (`log_pdf`), R2RelativeGaussianLikelihoodFactor (`evaluate_loglike`, point
         by point), UnaryR2RangeGaussianPriorFactor (the range likelihood with the first end pinned at the centre).
     a%03d_fd holds that finite difference for EVERY case (the script prints the largest disagreement with the analytic value),
     a%03d_mask [n] marks the rows the yardstick covers: rows at a range of exactly 0 (the reference divides by it) and
     mixture rows where the reference's `pdf` underflows to 0 are excluded -- the reference is undefined there -- and never
     more than 5 % of a case's rows.
 (b) whole graphs: `JointFactor.grad_x_log_pdf` (src/sampler/sampler_utils.py:101-118) at all 48 Manhattan-136 points of
     factor_density.npz and at the Plaza1-ADA points `plaza1ada_rows` of it (as many as the size of a committed file allows).
 (c) the reference's `Gaussian_kernel_stein_discrepancy` (src/utils/Statistics.py:216-245), seeded: a prior, two odometry
     factors, four ranges and an ambiguous-association factor over three poses and two landmarks (D = 13); n = 130 points
     truth + 0.15 N(0, 1) rounded to float32; P = diag(1 / (D var)).  Stored: samples, score, precision, ustats, vstats,
     off_ksd, p_u and the multinomial draws of its bootstrap (the generator re-seeded and the draws repeated).

    python tests/golden/make_factor_score_fixture.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_pipeline_fixture import REF, STUB, write_stubs  # noqa: E402

OUT = os.path.join(HERE, "factor_score.npz")
DENSITY = os.path.join(HERE, "factor_density.npz")
DATA = os.path.join(os.path.dirname(HERE), "data")
GRAPHS = {"manhattan136": "ManhattanPlaza136", "plaza1ada": "Plaza1ADA0.4EFG"}
PLAZA_ROWS = (0, 1, 6, 7, 12, 13)               # two points per noise scale of factor_density.npz
KSD_SEED, KSD_N, KSD_NBOOT = 20261019, 130, 200


def richardson(value, x, steps):
    """(4 D(h) - D(2h)) / 3 per coordinate, D the central difference of `value` ([n, w] -> [n]) with step steps[c]."""
    out = np.zeros_like(x)
    for c, h in enumerate(steps):
        def central(step):
            lo, hi = x.copy(), x.copy()
            lo[:, c] -= step
            hi[:, c] += step
            return (value(hi) - value(lo)) / (2.0 * step)
        out[:, c] = (4.0 * central(h) - central(2.0 * h)) / 3.0
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="nfisam_ref_")
    stubs = os.path.join(tmp, "stubs")
    write_stubs(stubs)
    try:
        import sklearn  # noqa: F401
    except ImportError:                                     # utils/Statistics.py imports it and never uses it
        os.makedirs(os.path.join(stubs, "sklearn"))
        with open(os.path.join(stubs, "sklearn", "__init__.py"), "w") as f:
            f.write(STUB)
    sys.path.insert(0, stubs)
    sys.path.insert(0, os.path.join(REF, "src"))
    sys.dont_write_bytecode = True
    import matplotlib
    matplotlib.use("Agg")
    import factors.Factors as F
    from geometry.TwoDimension import SE2Pose
    from sampler.sampler_utils import JointFactor
    from slam.RunBatch import graph_file_parser
    from slam.Variables import R2Variable, SE2Variable, VariableType
    from utils.Statistics import Gaussian_kernel_stein_discrepancy

    dens = np.load(DENSITY)
    out = {}
    X, Y = SE2Variable("X0"), SE2Variable("X1")
    L = [R2Variable("L%d" % i, variable_type=VariableType.Landmark) for i in range(4)]

    def ranges_of(x, pairs):
        return np.stack([np.sqrt(((x[:, a:a + 2] - x[:, b:b + 2]) ** 2).sum(1)) for a, b in pairs], 1)

    # ---- (a) ----------------------------------------------------------------------------------------------------------------
    worst_fd = 0.0
    for i, cls in enumerate(str(c) for c in dens["a_classes"]):
        p = [float(v) for v in dens["a%03d_params" % i]]
        x = dens["a%03d_x" % i].astype(np.float64)
        mask = np.ones(x.shape[0], dtype=bool)
        analytic = None
        if cls == "UnarySE2ApproximateGaussianPriorFactor":
            cov = np.array(p[3:]).reshape(3, 3)
            f = F.UnarySE2ApproximateGaussianPriorFactor(var=X, prior_pose=SE2Pose(*p[:3]), covariance=cov)
            value, steps, analytic = f.log_pdf, np.sqrt(np.diag(cov)), f.grad_x_log_pdf(x)
        elif cls == "SE2RelativeGaussianLikelihoodFactor":
            cov = np.array(p[3:]).reshape(3, 3)
            f = F.SE2RelativeGaussianLikelihoodFactor(var1=X, var2=Y, observation=SE2Pose(*p[:3]), covariance=cov)
            value, steps, analytic = f.log_pdf, np.tile(np.sqrt(np.diag(cov)), 2), f.grad_x_log_pdf(x)
        elif cls in ("SE2R2RangeGaussianLikelihoodFactor", "R2RangeGaussianLikelihoodFactor"):
            pose = cls.startswith("SE2")
            f = (F.SE2R2RangeGaussianLikelihoodFactor(var1=X, var2=L[0], observation=p[0], sigma=p[1]) if pose else
                 F.R2RangeGaussianLikelihoodFactor(var1=L[0], var2=L[1], observation=p[0], sigma=p[1]))
            mask = ranges_of(x, [(0, 3 if pose else 2)])[:, 0] > 0
            value, steps = f.log_pdf, np.full(x.shape[1], p[1])
            with np.errstate(all="ignore"):
                analytic = f.grad_x_log_pdf(x)
        elif cls == "AmbiguousDataAssociationFactor":
            k = int(p[0])
            f = F.AmbiguousDataAssociationFactor(observer_var=X, observed_vars=L[:k], weights=np.array(p[1:1 + k]),
                                                 binary_factor_class=F.SE2R2RangeGaussianLikelihoodFactor,
                                                 observation=p[1 + k], sigma=p[2 + k])
            mask = (ranges_of(x, [(0, 3 + 2 * j) for j in range(k)]) > 0).all(1) & (f.pdf(x) > 0)
            value, steps = f.log_pdf, np.full(x.shape[1], p[2 + k])
            with np.errstate(all="ignore"):
                analytic = f.grad_x_log_pdf(x)
        elif cls == "BinaryFactorWithNullHypo":
            f = F.BinaryFactorWithNullHypo(var1=X, var2=L[0], weights=np.array(p[:2]),
                                           binary_factor_class=F.SE2R2RangeGaussianLikelihoodFactor, observation=p[2],
                                           sigma=p[3], null_sigma_scale=p[4])
            mask = (ranges_of(x, [(0, 3)])[:, 0] > 0) & (f.pdf(x) > 0)
            value, steps = f.log_pdf, np.full(x.shape[1], p[3])
            with np.errstate(all="ignore"):
                analytic = f.grad_x_log_pdf(x)
        elif cls == "UnaryR2GaussianPriorFactor":
            cov = np.array(p[2:]).reshape(2, 2)
            f = F.UnaryR2GaussianPriorFactor(var=L[0], mu=np.array(p[:2]), covariance=cov)
            value, steps = f.log_pdf, np.sqrt(np.diag(cov))
        elif cls == "R2RelativeGaussianLikelihoodFactor":
            cov = np.array(p[2:]).reshape(2, 2)
            f = F.R2RelativeGaussianLikelihoodFactor(var1=L[0], var2=L[1], observation=np.array(p[:2]), covariance=cov)
            value = lambda pts, f=f: np.array([float(f.evaluate_loglike(r)) for r in pts])
            steps = np.tile(np.sqrt(np.diag(cov)), 2)
        elif cls == "UnaryR2RangeGaussianPriorFactor":
            f = F.R2RangeGaussianLikelihoodFactor(var1=L[0], var2=L[1], observation=p[2], sigma=p[3])
            centre = np.array(p[:2], dtype=np.float32).astype(np.float64)     # what the density fixture pinned
            value = lambda pts, f=f, centre=centre: f.log_pdf(np.concatenate([np.tile(centre, (pts.shape[0], 1)), pts], 1))
            steps = np.full(2, p[3])
            mask = np.sqrt(((x - centre) ** 2).sum(1)) > 0
        else:
            raise KeyError(cls)
        mask = np.asarray(mask, dtype=bool)
        with np.errstate(all="ignore"):
            fd = richardson(lambda pts: np.asarray(value(pts), dtype=np.float64).reshape(-1), x, 1e-3 * steps)
        ref = np.asarray(analytic if analytic is not None else fd, dtype=np.float64)
        assert ref.shape == x.shape and np.all(np.isfinite(ref[mask])), (i, cls)
        assert (~mask).sum() <= 0.05 * mask.size, (i, cls, int((~mask).sum()), mask.size)
        ref[~mask] = 0.0
        fd[~mask] = 0.0
        assert np.all(np.isfinite(fd)), (i, cls)
        dis = float(np.max(np.abs(fd - ref)[mask] / (np.abs(ref[mask]) + 1.0)))
        worst_fd = max(worst_fd, dis)
        print("a%03d %-42s rows %2d (masked %d)  %s   |fd - analytic| / (|analytic| + 1) = %.3g"
              % (i, cls, x.shape[0], int((~mask).sum()), "reference" if analytic is not None else "richardson", dis))
        out["a%03d_ref" % i], out["a%03d_fd" % i], out["a%03d_mask" % i] = ref, fd, mask
        out["a%03d_analytic" % i] = np.array(analytic is not None)
    print("largest disagreement between the finite difference and the analytic value: %.3g" % worst_fd)

    # ---- (b) ----------------------------------------------------------------------------------------------------------------
    for key, folder in GRAPHS.items():
        nodes, truth, factors = graph_file_parser(data_file=os.path.join(DATA, folder, "factor_graph.fg"), data_format="fg",
                                                  prior_cov_scale=0.1)
        assert [str(v.name) for v in nodes] == [str(s) for s in dens[key + "_vars"]]
        joint = JointFactor(factors, nodes)
        rows = np.arange(dens[key + "_x"].shape[0]) if key == "manhattan136" else np.array(PLAZA_ROWS)
        x = dens[key + "_x"][rows].astype(np.float64)
        g = np.asarray(joint.grad_x_log_pdf(x), dtype=np.float64)
        assert g.shape == x.shape and np.all(np.isfinite(g)), "non-finite reference score: choose other rows"
        out[key + "_rows"], out[key + "_score"] = rows.astype(np.int32), g
        print(key, len(factors), "factors", g.shape, "largest |score| %.3g" % np.abs(g).max())

    # ---- (c) ----------------------------------------------------------------------------------------------------------------
    P = [SE2Variable("X%d" % i) for i in range(3)]
    M = [R2Variable("L%d" % i, variable_type=VariableType.Landmark) for i in range(2)]
    truth = np.array([0.0, 0.0, 0.0, 2.0, 0.0, 0.5, 3.5, 1.0, 1.2, 2.0, 3.0, 5.0, -1.0])
    odo = np.diag([0.04, 0.04, 0.01])
    factors = [F.UnarySE2ApproximateGaussianPriorFactor(var=P[0], prior_pose=SE2Pose(0.0, 0.0, 0.0),
                                                        covariance=np.diag([0.01, 0.01, 0.0025])),
               F.SE2RelativeGaussianLikelihoodFactor(var1=P[0], var2=P[1], observation=SE2Pose(2.0, 0.0, 0.5), covariance=odo),
               F.SE2RelativeGaussianLikelihoodFactor(var1=P[1], var2=P[2], observation=SE2Pose(1.8, 0.16, 0.7), covariance=odo)]

    def dist(a, b):
        return float(np.sqrt(((truth[a:a + 2] - truth[b:b + 2]) ** 2).sum()))
    for pose, lm in ((0, 0), (1, 0), (1, 1), (2, 1)):
        factors.append(F.SE2R2RangeGaussianLikelihoodFactor(var1=P[pose], var2=M[lm], observation=dist(3 * pose, 9 + 2 * lm),
                                                            sigma=0.3))
    factors.append(F.AmbiguousDataAssociationFactor(observer_var=P[2], observed_vars=M, weights=np.array([0.5, 0.5]),
                                                    binary_factor_class=F.SE2R2RangeGaussianLikelihoodFactor,
                                                    observation=dist(6, 9), sigma=0.3))
    joint = JointFactor(factors, P + M)
    rng = np.random.RandomState(KSD_SEED)
    samples = (truth + 0.15 * rng.randn(KSD_N, truth.size)).astype(np.float32).astype(np.float64)
    precision = 1.0 / (truth.size * samples.var(0))
    np.random.seed(KSD_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        ustats, p_u, off_ksd, vstats = Gaussian_kernel_stein_discrepancy(joint, np.diag(precision), samples, nboot=KSD_NBOOT)
    np.random.seed(KSD_SEED)
    draws = np.stack([np.random.multinomial(KSD_N, np.ones(KSD_N) / KSD_N) for _ in range(KSD_NBOOT)])
    boot = np.array([(w / KSD_N - 1.0 / KSD_N) @ off_ksd @ (w / KSD_N - 1.0 / KSD_N) for w in draws])
    assert abs(np.mean(boot >= ustats) - p_u) < 1e-12, "the redrawn multinomials are not the ones the reference used"
    score = np.asarray(joint.grad_x_log_pdf(samples), dtype=np.float64)
    assert np.all(np.isfinite(score)) and np.all(np.isfinite(off_ksd))
    out.update(ksd_samples=samples.astype(np.float32), ksd_score=score, ksd_precision=precision, ksd_ustats=np.array(ustats),
               ksd_vstats=np.array(vstats), ksd_off=off_ksd, ksd_p_u=np.array(p_u), ksd_draws=draws.astype(np.int32),
               ksd_truth=truth, ksd_factors=np.array([str(f.__class__.__name__) + " " + " ".join(str(v.name) for v in f.vars)
                                                      for f in factors]))
    print("ksd: ustats %.6g  vstats %.6g  p_u %.3g" % (ustats, vstats, p_u))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
