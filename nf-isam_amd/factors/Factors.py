"""factors.Factors — the factor types that feed the flow hot path in the range-only SLAM
configurations (reference: src/factors/Factors.py, 3489 lines).

Only what the clique training-batch simulator needs is restated: the class hierarchy used for
dispatch (`PriorFactor`, `BinaryFactor`, ...), `.fg` text (de)serialisation, and **batched**
`sample` methods for
    UnarySE2ApproximateGaussianPriorFactor   (reference :682-849)
    SE2RelativeGaussianLikelihoodFactor       (reference :1095-1478)
    SE2R2RangeGaussianLikelihoodFactor        (reference :2510-2751)
    AmbiguousDataAssociationFactor            (reference :3043-3298; k-way mixture over candidate landmarks)
    BinaryFactorWithNullHypo                  (reference :3300-3462; possibly-outlier measurement)
    UnaryR2GaussianPriorFactor, UnaryR2RangeGaussianPriorFactor, R2RelativeGaussianLikelihoodFactor,
    R2RangeGaussianLikelihoodFactor           (reference :362, :451, :912, :2026; the toy range-only examples)
The reference draws noise with TransportMaps' `GaussianDistribution.rvs` and then loops over
samples building `SE2Pose` objects; here the noise comes from numpy's global RNG (seeded by the
example scripts exactly like the reference's) and the pose algebra is vectorised
(geometry.TwoDimension).

Density evaluation: every class has `log_pdf(x)` / `pdf(x)` (x: [n, sum of the variables' dims], columns in
`factor.vars` order, float64 throughout), vectorised over n with no `SE2Pose` objects:
    SE(2) prior / relative pose   N(Log(dT); 0, Sigma) + log|det dLog|, det = th^2 / (4 sin^2(th/2)), 1 for |th| < 1e-5
                                  (reference :823-827, :1443-1448; geometry/TwoDimension.py:405-441)
    range factors                 N(|a_xy - b_xy| - d; 0, sigma^2)              (reference :2724-2730, :2195-2201)
    mixtures                      log sum_k w_k p_k                            (reference :3126-3133)
    R2 Gaussian prior / relative  the multivariate normal of x - mu / of var2 - var1 - observation (reference :373, :1070-1074)
    R2 range prior                N(|x - center| - mu; 0, sigma^2): the density of what `sample` draws.  The reference's only
                                  body for it (:2301-2303, `evaluate_loglike`) subtracts mu inside the norm and is no range
                                  density; the range likelihood with one end pinned at the centre is what is restated.
One deliberate difference: the reference's mixture takes `np.log` of a sum of `exp`s, which is -inf far from every
component; here mixtures use log-sum-exp and stay finite (equal wherever the reference is finite).  The log map uses the
half-angle form (th/2) cot(th/2), which does not cancel for small th.  `density_record()` returns the factor's row of the
device table of `nfisam_factor_graph_log_density` (include/nfisam_hip.h).

Scores: the seven classes with a `density_record` have `grad_x_log_pdf(x)` -> [n, dim] float64, the derivative of the
class's own `log_pdf` (of its smooth formula: small-angle series of the log map below |w| = 0.2), with the conventions of the
device entry `nfisam_factor_graph_score`: the zero vector at a range of exactly 0, softmax weights for mixtures.
"""
from typing import Iterable, List, Union

import numpy as np

from geometry.TwoDimension import SE2Pose, se2_compose, se2_exp, se2_inverse, wrap_pi
from slam.Variables import R1Variable, R2Variable, SE2Variable, Variable, VariableType


# ---- class hierarchy used for dispatch ---------------------------------------------------------
class Factor(object):
    @property
    def vars(self) -> List[Variable]:
        raise NotImplementedError

    @property
    def dim(self) -> int:
        return sum(v.dim for v in self.vars)

    @property
    def is_gaussian(self) -> bool:
        return False

    def pdf(self, x: np.ndarray) -> np.ndarray:
        return np.exp(self.log_pdf(x))

    def __str__(self) -> str:
        return "Factor " + self.__class__.__name__ + " " + " ".join(str(v.name) for v in self.vars)

    @classmethod
    def construct_from_text(cls, line: str, variables: Iterable[Variable]) -> "Factor":
        """`Factor <ClassName> <args...>` -> instance (reference :42-52)."""
        tok = line.strip().split()
        if tok[0] == "Factor":
            tok = tok[1:]
        klass = _FACTOR_CLASSES.get(tok[0])
        if klass is None:
            raise NotImplementedError("factor type %s is outside the rebuilt scope (SURVEY.md §8 f-2)" % tok[0])
        return klass.construct_from_text(" ".join(tok), variables)


class UnaryFactor(Factor):
    @property
    def var(self) -> Variable:
        return self.vars[0]


class BinaryFactor(Factor):
    @property
    def var1(self) -> Variable:
        return self.vars[0]

    @property
    def var2(self) -> Variable:
        return self.vars[1]


class PriorFactor(Factor):
    def sample(self, num_samples: int, **kwargs) -> np.ndarray:
        raise NotImplementedError


class LikelihoodFactor(Factor):
    @property
    def observation(self) -> np.ndarray:
        raise NotImplementedError


class ExplicitPriorFactor(PriorFactor):
    pass


class ImplicitPriorFactor(PriorFactor):
    """A prior that is only available through sampling, e.g. a trained clique density."""


class OdomFactor(object):
    """Marker of relative-motion factors between consecutive poses (reference :908)."""


class KWayFactor(Factor):
    @property
    def root_var(self) -> Variable:
        raise NotImplementedError

    @property
    def child_vars(self) -> List[Variable]:
        raise NotImplementedError


class BinaryFactorWithNullHypo(BinaryFactor):
    """Defined below, after the mixture base (reference :3300-3462); declared here for the dispatch order."""


def _gaussian_noise(cov_chol: np.ndarray, n: int) -> np.ndarray:
    return np.random.standard_normal((n, cov_chol.shape[0])) @ cov_chol.T


# ---- densities (float64, vectorised over the rows of x) -------------------------------------------------
_LOG_2PI = float(np.log(2.0 * np.pi))


def _gaussian_log_norm(covariance: np.ndarray) -> float:
    covariance = np.atleast_2d(np.asarray(covariance, dtype=np.float64))
    return float(-0.5 * (covariance.shape[0] * _LOG_2PI + np.linalg.slogdet(covariance)[1]))


def _quad_form(d: np.ndarray, precision: np.ndarray) -> np.ndarray:
    return np.einsum("ni,ij,nj->n", d, precision, d)


def _sym_upper(precision: np.ndarray) -> List[float]:
    """Upper triangle (row-major) of the symmetrised precision: the device adds each off-diagonal entry twice."""
    ps = 0.5 * (precision + precision.T)
    return [float(ps[r, c]) for r in range(ps.shape[0]) for c in range(r, ps.shape[0])]


def _se2_tangent_log_pdf(tx, ty, w, precision, log_norm) -> np.ndarray:
    """log N(Log(dT); 0, Sigma) + log|det dLog/d(x, y, theta)| for dT = (tx, ty, w), w in [-pi, pi)
    (reference geometry/TwoDimension.py:405-418 log_map, :437-441 det_grad_x_logmap)."""
    small = np.abs(w) < 1e-10                    # a = 1 - w^2 / 12 is 1 there; the off-diagonal w / 2 of V^-1 is kept (the
    half = 0.5 * np.where(small, 1.0, w)         # reference's identity drops |w| |t| / 2: 1e-10 relative, csrc/factor_model.h)
    a = np.where(small, 1.0, half * np.cos(half) / np.sin(half))
    b = 0.5 * w
    v = np.stack([a * tx + b * ty, -b * tx + a * ty, w], axis=1)
    flat = np.abs(w) < 1e-5
    h = 0.5 * np.where(flat, 1.0, w)
    log_det = np.where(flat, 0.0, 2.0 * np.log(np.abs(h / np.sin(h))))
    return log_norm - 0.5 * _quad_form(v, precision) + log_det


_SERIES_H = 0.1


def _log_map_terms(w):
    """a = h cot h (h = w / 2), da / dw = (cot h - h / sin^2 h) / 2 and d/dw of the log-det term 2 log|h / sin h|,
    1 / h - cot h.  The two derivatives are differences of terms of size 1 / h that leave h / 3: the plain forms lose
    1.5 eps / h^2 relative.  Below |h| = 0.1 the Taylor series through h^9 replace them: there the plain forms have lost
    two digits (1.7e-14) and the first dropped series terms are 3.9e-15 and 6.5e-16 relative, so neither side of the switch
    is more than about two digits worse than the other (the same switch as csrc/factor_model.h)."""
    h = 0.5 * np.asarray(w, dtype=np.float64)
    ser = np.abs(h) < _SERIES_H
    h2 = np.where(ser, h * h, 0.0)
    a_s = 1.0 - h2 * (1.0 / 3.0 + h2 * (1.0 / 45.0 + h2 * (2.0 / 945.0 + h2 * (1.0 / 4725.0 + h2 * (2.0 / 93555.0)))))
    da_s = -h * (1.0 / 3.0 + h2 * (2.0 / 45.0 + h2 * (2.0 / 315.0 + h2 * (4.0 / 4725.0 + h2 * (2.0 / 18711.0)))))
    dl_s = h * (1.0 / 3.0 + h2 * (1.0 / 45.0 + h2 * (2.0 / 945.0 + h2 * (1.0 / 4725.0 + h2 * (2.0 / 93555.0)))))
    hp = np.where(ser, 1.0, h)
    sh, ch = np.sin(hp), np.cos(hp)
    cot = ch / sh
    return (np.where(ser, a_s, hp * cot), np.where(ser, da_s, 0.5 * (cot - hp / (sh * sh))),
            np.where(ser, dl_s, 1.0 / hp - cot))


def _se2_tangent_score(tx, ty, w, precision):
    """d/d(tx, ty, w) of `_se2_tangent_log_pdf`: of its smooth formula everywhere (the value's |w| < 1e-10 and |w| < 1e-5
    branches are flat spots of that width and get no derivative-zero plateaus)."""
    a, da, dl = _log_map_terms(w)
    h = 0.5 * w
    P = 0.5 * (precision + precision.T)
    vx, vy = a * tx + h * ty, a * ty - h * tx
    gvx = -(P[0, 0] * vx + P[0, 1] * vy + P[0, 2] * w)
    gvy = -(P[0, 1] * vx + P[1, 1] * vy + P[1, 2] * w)
    gvw = -(P[0, 2] * vx + P[1, 2] * vy + P[2, 2] * w)
    return (a * gvx - h * gvy, h * gvx + a * gvy,
            gvw + gvx * (da * tx + 0.5 * ty) + gvy * (da * ty - 0.5 * tx) + dl)


_SERIES2_H = 0.3


def _log_map_curvature(w, a):
    """The second derivatives in w of a = h cot h and of the log-det term: a'' = (a - 1) / (2 sin^2 h) and
    l'' = (1 / sin^2 h - 1 / h^2) / 2, differences of terms of size 1 / h^2 that leave -1/6 and 1/6: the plain forms lose
    3 eps / h^2 and 6 eps / h^2 relative.  Below |h| = 0.3 the Taylor series through h^16 replace them: there the plain
    forms have lost 33 and 67 roundings and the first dropped series terms are under half a rounding (the same switch and
    the same balance as csrc/factor_model.h)."""
    h = 0.5 * np.asarray(w, dtype=np.float64)
    ser = np.abs(h) < _SERIES2_H
    h2 = np.where(ser, h * h, 0.0)
    dda_s = -(1.0 / 6.0 + h2 * (1.0 / 15.0 + h2 * (1.0 / 63.0 + h2 * (2.0 / 675.0 + h2 * (1.0 / 2079.0 + h2 * (
        1382.0 / 19348875.0 + h2 * (2.0 / 200475.0 + h2 * (14468.0 / 10854718875.0 + h2 * (43867.0 / 254766637125.0)))))))))
    ddl_s = 1.0 / 6.0 + h2 * (1.0 / 30.0 + h2 * (1.0 / 189.0 + h2 * (1.0 / 1350.0 + h2 * (1.0 / 10395.0 + h2 * (
        691.0 / 58046625.0 + h2 * (2.0 / 1403325.0 + h2 * (3617.0 / 21709437750.0 + h2 * (43867.0 / 2292899734125.0))))))))
    hp = np.where(ser, 1.0, h)
    is2 = 1.0 / np.sin(hp) ** 2
    return np.where(ser, dda_s, 0.5 * (a - 1.0) * is2), np.where(ser, ddl_s, 0.5 * (is2 - 1.0 / (hp * hp)))


def _se2_tangent_hvp(tx, ty, w, precision, vtx, vty, vw):
    """(gtx, gty, and the derivative of `_se2_tangent_score` along (vtx, vty, vw)): the Hessian of the tangent density times
    a direction, line by line the derivative of the score (csrc/factor_model.h: se2_tangent_hvp)."""
    a, da, dl = _log_map_terms(w)
    dda, ddl = _log_map_curvature(w, a)
    h = 0.5 * w
    P = 0.5 * (precision + precision.T)
    vx, vy = a * tx + h * ty, a * ty - h * tx
    gvx = -(P[0, 0] * vx + P[0, 1] * vy + P[0, 2] * w)
    gvy = -(P[0, 1] * vx + P[1, 1] * vy + P[1, 2] * w)
    jx, jy = da * tx + 0.5 * ty, da * ty - 0.5 * tx
    dvx, dvy = a * vtx + h * vty + jx * vw, a * vty - h * vtx + jy * vw
    dgvx = -(P[0, 0] * dvx + P[0, 1] * dvy + P[0, 2] * vw)
    dgvy = -(P[0, 1] * dvx + P[1, 1] * dvy + P[1, 2] * vw)
    dgvw = -(P[0, 2] * dvx + P[1, 2] * dvy + P[2, 2] * vw)
    return (a * gvx - h * gvy, h * gvx + a * gvy,
            a * dgvx - h * dgvy + (da * gvx - 0.5 * gvy) * vw,
            h * dgvx + a * dgvy + (0.5 * gvx + da * gvy) * vw,
            dgvw + dgvx * jx + dgvy * jy + gvx * (dda * vw * tx + da * vtx + 0.5 * vty)
            + gvy * (dda * vw * ty + da * vty - 0.5 * vtx) + ddl * vw)


def _range_log_pdf(r, d, sigma):
    delta = r - d
    return _gaussian_log_norm(sigma ** 2) - 0.5 * delta * delta * (1.0 / sigma ** 2)


def _range_score(diff, r, d, sigma):
    """d/d(ta) of log N(|ta - tb| - d; 0, sigma^2) (d/d(tb) is its negative): -(r - d) / sigma^2 (ta - tb) / r, and the
    zero vector at r = 0 exactly, where the range has no direction."""
    c = np.zeros_like(r)
    ok = r > 0
    c[ok] = -(r[ok] - d) / (sigma ** 2 * r[ok])
    return c[:, None] * diff


def _range_hess(diff, r, d, sigma):
    """The block in ta of the Hessian of log N(|ta - tb| - d; 0, sigma^2), [n, 2, 2]: with u = (ta - tb) / r and
    delta = r - d it is -[u u' + (delta / r) (I - u u')] / sigma^2 (the tb-tb block is the same, the ta-tb block its
    negative), and the zero block at r = 0 exactly, like the score."""
    out = np.zeros((r.shape[0], 2, 2))
    ok = r > 0
    u = diff[ok] / r[ok][:, None]
    uu = u[:, :, None] * u[:, None, :]
    k = ((r[ok] - d) / r[ok])[:, None, None]
    out[ok] = -(uu + k * (np.eye(2) - uu)) / sigma ** 2
    return out


def _as_points(x, width: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != width:
        raise ValueError("x must be [n, %d], got %s" % (width, tuple(x.shape)))
    return x


def _mat3(tok, start):
    return np.array([[float(tok[start + 3 * r + c]) for c in range(3)] for r in range(3)])


# ---- SE(2) prior -----------------------------------------------------------------------------
class UnarySE2ApproximateGaussianPriorFactor(ExplicitPriorFactor, UnaryFactor):
    """x = prior_pose * Exp(eps), eps ~ N(0, covariance) in the tangent space."""

    def __init__(self, var: Variable, prior_pose: Union[SE2Pose, np.ndarray], covariance: np.ndarray,
                 correlated_R_t: bool = True):
        if not isinstance(prior_pose, SE2Pose):
            prior_pose = SE2Pose(*prior_pose)
        assert var.dim == 3 and np.shape(covariance) == (3, 3)
        self._vars = [var]
        self._prior_pose = prior_pose
        self._covariance = np.array(covariance, dtype=np.float64)
        self._chol = np.linalg.cholesky(self._covariance)
        self._precision = np.linalg.inv(self._covariance)
        self._log_norm = _gaussian_log_norm(self._covariance)
        self._correlated_R_t = correlated_R_t

    @property
    def vars(self):
        return self._vars

    @property
    def observation(self):
        return self._prior_pose.array

    @property
    def mu(self):
        return self.observation

    @property
    def covariance(self):
        return self._covariance

    @property
    def is_gaussian(self):
        return True

    def sample(self, num_samples: int, **kwargs) -> np.ndarray:
        noise = _gaussian_noise(self._chol, num_samples)
        if self._correlated_R_t:
            return se2_compose(self._prior_pose.array, se2_exp(noise))
        theta = np.random.vonmises(mu=0.0, kappa=1.0 / self._covariance[2, 2], size=num_samples)
        out = np.empty((num_samples, 3))
        out[:, :2] = self._prior_pose.array[:2] + noise[:, :2]
        out[:, 2] = (self._prior_pose.theta + theta + np.pi) % (2 * np.pi) - np.pi
        return out

    def _residual(self, x):
        """-> (tx, ty, w) = prior^-1 * T, and (cos, sin) of the prior's heading: the rotation a gradient goes back through."""
        x = _as_points(x, 3)
        px, py, pth = self._prior_pose.array
        c, s = np.cos(pth), np.sin(pth)
        dx, dy = x[:, 0] - px, x[:, 1] - py
        w = wrap_pi(wrap_pi(-pth) + wrap_pi(x[:, 2]))
        return c * dx + s * dy, -s * dx + c * dy, w, c, s

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """Density in (x, y, theta) of the pose: the tangent Gaussian of prior^-1 * T times the Jacobian of Log
        (reference :823-827)."""
        tx, ty, w, c, s = self._residual(x)
        return _se2_tangent_log_pdf(tx, ty, w, self._precision, self._log_norm)

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d log_pdf / d(x, y, theta), [n, 3] float64 (reference :829-850); the heading wrap has derivative 1."""
        tx, ty, w, c, s = self._residual(x)
        gtx, gty, gw = _se2_tangent_score(tx, ty, w, self._precision)
        return np.stack([c * gtx - s * gty, s * gtx + c * gty, gw], 1)

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d^2 log_pdf / d(x, y, theta)^2, [n, 3, 3] float64: column k is the derivative of `grad_x_log_pdf` along e_k."""
        tx, ty, w, c, s = self._residual(x)
        one, zero = np.ones_like(w), np.zeros_like(w)
        out = np.empty((w.shape[0], 3, 3))
        for k, (vx, vy, vw) in enumerate(((one, zero, zero), (zero, one, zero), (zero, zero, one))):
            _, _, htx, hty, hw = _se2_tangent_hvp(tx, ty, w, self._precision, c * vx + s * vy, c * vy - s * vx, vw)
            out[:, :, k] = np.stack([c * htx - s * hty, s * htx + c * hty, hw], 1)
        return out

    def density_record(self) -> dict:
        return dict(code="PRIOR_SE2", a=self.var, b=None, cand=[],
                    p=[float(t) for t in self._prior_pose.array] + _sym_upper(self._precision) + [self._log_norm])

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        var = {v.name: v for v in variables}[tok[1]]
        mat = _mat3(tok, 6)
        if tok[5] == "covariance":
            cov = mat
        elif tok[5] == "information":
            cov = np.linalg.inv(mat)
        else:
            raise ValueError("Either covariance or information should be specified")
        return cls(var=var, prior_pose=SE2Pose(float(tok[2]), float(tok[3]), float(tok[4])), covariance=cov)

    def __str__(self):
        c = self._covariance
        return " ".join(["Factor", self.__class__.__name__, str(self.var.name)] + [str(v) for v in self.mu] +
                        ["covariance"] + [str(c[r, k]) for r in range(3) for k in range(3)])


# ---- SE(2) relative pose (odometry / loop closure) -------------------------------------------------
class SE2RelativeGaussianLikelihoodFactor(LikelihoodFactor, BinaryFactor, OdomFactor):
    """T_j = T_i * (observation * Exp(eps)), eps ~ N(0, covariance)."""
    measurement_dim = 3
    measurement_type = SE2Variable

    def __init__(self, var1: Variable, var2: Variable, observation: Union[SE2Pose, np.ndarray],
                 covariance: np.ndarray = None, correlated_R_t: bool = True, information: np.ndarray = None):
        if isinstance(observation, (np.ndarray, list, tuple)):
            observation = SE2Pose(*observation)
        if covariance is None:
            covariance = np.linalg.inv(information)
        if not (var1.dim == var2.dim == 3):
            raise ValueError("Dimensionality of poses, relative pose and observation must be 3")
        self._vars = [var1, var2]
        self._observation = observation
        self._covariance = np.array(covariance, dtype=np.float64)
        self._chol = np.linalg.cholesky(self._covariance)
        self._precision = np.linalg.inv(self._covariance)
        self._log_norm = _gaussian_log_norm(self._covariance)
        self._correlated_Rt = correlated_R_t
        self._observation_var = SE2Variable(name="O" + str(var1.name) + str(var2.name),
                                            variable_type=VariableType.Measurement)

    @property
    def vars(self):
        return self._vars

    @property
    def observation_var(self):
        return self._observation_var

    @property
    def circular_dim_list(self):
        return self._observation_var.circular_dim_list

    @property
    def covariance(self):
        return self._covariance

    @property
    def noise_cov(self):
        return self._covariance

    @property
    def observation(self) -> np.ndarray:
        return self._observation.array

    def _noisy_relative(self, base: np.ndarray, n: int) -> np.ndarray:
        if not self._correlated_Rt:
            raise NotImplementedError("correlated_R_t=False is not used by the shipped configurations")
        return se2_compose(base, se2_exp(_gaussian_noise(self._chol, n)))

    def sample(self, var1: Union[np.ndarray, None] = None, var2: Union[np.ndarray, None] = None) -> np.ndarray:
        """var2 given -> var1 samples; var1 given -> var2 samples; both -> simulated observations."""
        if var1 is None:
            if var2 is None:
                raise ValueError("Samples of at least one variable must be specified")
            rel = self._noisy_relative(self.observation, var2.shape[0])
            return se2_compose(var2, se2_inverse(rel))
        if var2 is None:
            rel = self._noisy_relative(self.observation, var1.shape[0])
            return se2_compose(var1, rel)
        if var1.shape != var2.shape or var1.shape[1] != 3:
            raise ValueError("Dimensionality of variable 1 or variable 2 is wrong")
        return self._noisy_relative(se2_compose(se2_inverse(var1), var2), var1.shape[0])

    def _residual(self, x):
        """-> (tx, ty, w) = observation^-1 * (T_i^-1 * T_j), then what a gradient goes back through: (cos, sin) of the
        observation's heading and of pose i's, and (ux, uy), the difference of the positions in pose i's frame."""
        x = _as_points(x, 6)
        ox, oy, oth = self.observation
        ci, si = np.cos(x[:, 2]), np.sin(x[:, 2])
        dx, dy = x[:, 3] - x[:, 0], x[:, 4] - x[:, 1]
        ux, uy = ci * dx + si * dy, -si * dx + ci * dy
        rx, ry = ux - ox, uy - oy
        co, so = np.cos(oth), np.sin(oth)
        w = wrap_pi(wrap_pi(-oth) + wrap_pi(wrap_pi(-wrap_pi(x[:, 2])) + wrap_pi(x[:, 5])))
        return co * rx + so * ry, -so * rx + co * ry, w, co, so, ci, si, ux, uy

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """Density of x = [T_i | T_j]: the tangent Gaussian of observation^-1 * (T_i^-1 * T_j) times the Jacobian of Log
        (reference :1443-1448)."""
        tx, ty, w = self._residual(x)[:3]
        return _se2_tangent_log_pdf(tx, ty, w, self._precision, self._log_norm)

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d log_pdf / d[T_i | T_j], [n, 6] float64 (reference :1450-1478)."""
        tx, ty, w, co, so, ci, si, ux, uy = self._residual(x)
        gtx, gty, gw = _se2_tangent_score(tx, ty, w, self._precision)
        grx, gry = co * gtx - so * gty, so * gtx + co * gty
        gx, gy = ci * grx - si * gry, si * grx + ci * gry           # d/d(x_j, y_j)
        return np.stack([-gx, -gy, grx * uy - gry * ux - gw, gx, gy, gw], 1)

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d^2 log_pdf / d[T_i | T_j]^2, [n, 6, 6] float64: column k is the derivative of `grad_x_log_pdf` along e_k
        (d u / d th_i = (uy, -ux); the rotation back into the world frame turns with th_i)."""
        tx, ty, w, co, so, ci, si, ux, uy = self._residual(x)
        out = np.empty((w.shape[0], 6, 6))
        for k in range(6):
            v = [np.full_like(w, float(j == k)) for j in range(6)]
            ddx, ddy = v[3] - v[0], v[4] - v[1]
            dux, duy = ci * ddx + si * ddy + uy * v[2], ci * ddy - si * ddx - ux * v[2]
            gtx, gty, htx, hty, hw = _se2_tangent_hvp(tx, ty, w, self._precision, co * dux + so * duy, co * duy - so * dux,
                                                      v[5] - v[2])
            grx, gry = co * gtx - so * gty, so * gtx + co * gty
            hrx, hry = co * htx - so * hty, so * htx + co * hty
            hx = ci * hrx - si * hry - (si * grx + ci * gry) * v[2]
            hy = si * hrx + ci * hry + (ci * grx - si * gry) * v[2]
            out[:, :, k] = np.stack([-hx, -hy, hrx * uy + grx * duy - hry * ux - gry * dux - hw, hx, hy, hw], 1)
        return out

    def density_record(self) -> dict:
        return dict(code="REL_SE2", a=self.var1, b=self.var2, cand=[],
                    p=[float(t) for t in self.observation] + _sym_upper(self._precision) + [self._log_norm])

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        name_to_var = {v.name: v for v in variables}
        obs = SE2Pose(float(tok[3]), float(tok[4]), float(tok[5]))
        return cls(var1=name_to_var[tok[1]], var2=name_to_var[tok[2]], observation=obs, **{tok[6]: _mat3(tok, 7)})

    def __str__(self):
        c = self._covariance
        return " ".join(["Factor", self.__class__.__name__] + [str(v.name) for v in self.vars] +
                        [str(v) for v in self.observation] + ["covariance"] +
                        [str(c[r, k]) for r in range(3) for k in range(3)])


# ---- range between an SE(2)/R2 variable and an R2/SE(2) variable ---------------------------------
class SE2R2RangeGaussianLikelihoodFactor(LikelihoodFactor, BinaryFactor):
    """|t_2 - t_1| = observation + N(0, sigma^2); sampling one end from the other puts it on a
    ring of uniformly random bearing (the source of the non-Gaussian posteriors)."""
    measurement_dim = 1
    measurement_type = R1Variable

    def __init__(self, var1: Variable, var2: Variable, observation: Union[np.ndarray, float], sigma: float = 1.0):
        self._vars = [var1, var2]
        self._observation = observation if isinstance(observation, np.ndarray) else np.array([observation])
        self._sigma = float(sigma)
        self._observation_var = R1Variable(name="O" + str(var1.name) + str(var2.name),
                                           variable_type=VariableType.Measurement)

    @property
    def vars(self):
        return self._vars

    @property
    def observation_var(self):
        return self._observation_var

    @property
    def circular_dim_list(self):
        return self._observation_var.circular_dim_list

    @property
    def observation(self) -> np.ndarray:
        return self._observation

    @property
    def sigma(self) -> float:
        return self._sigma

    def _ring(self, centers: np.ndarray) -> np.ndarray:
        n = centers.shape[0]
        r = self._observation[0] + self._sigma * np.random.standard_normal(n)
        phi = np.random.uniform(-np.pi, np.pi, n)
        return centers + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)

    def sample_var2_from_var1(self, var1_samples: np.ndarray) -> np.ndarray:
        if var1_samples.ndim != 2 or var1_samples.shape[1] != self.var1.dim:
            raise ValueError("The dimensionality of variable 1 is wrong")
        return self._ring(var1_samples[:, self.var1.t_dim_indices])

    def sample_var1_from_var2(self, var2_samples: np.ndarray) -> np.ndarray:
        if var2_samples.ndim != 2 or var2_samples.shape[1] != self.var2.dim:
            raise ValueError("The dimensionality of variable 2 is wrong")
        return self._ring(var2_samples[:, self.var2.t_dim_indices])

    def sample_observations(self, var1_samples: np.ndarray, var2_samples: np.ndarray) -> np.ndarray:
        d = var2_samples[:, self.var2.t_dim_indices] - var1_samples[:, self.var1.t_dim_indices]
        n = var1_samples.shape[0]
        return (np.sqrt((d ** 2).sum(1)) + self._sigma * np.random.standard_normal(n)).reshape(n, 1)

    def pdf(self, x: np.ndarray) -> np.ndarray:
        """Likelihood of the stored observation given joint samples x = [var1 | var2] (reference :2680-2700)."""
        d1 = self.var1.dim
        t1 = x[:, :d1][:, self.var1.t_dim_indices]
        t2 = x[:, d1:][:, self.var2.t_dim_indices]
        r = np.sqrt(((t2 - t1) ** 2).sum(1))
        return np.exp(-0.5 * ((r - self._observation[0]) / self._sigma) ** 2) / (np.sqrt(2 * np.pi) * self._sigma)

    def _residual(self, x):
        """-> (x, the position columns of var1 and of var2, t_1 - t_2, |t_1 - t_2|)."""
        x = _as_points(x, self.var1.dim + self.var2.dim)
        i1 = np.asarray(self.var1.t_dim_indices)
        i2 = self.var1.dim + np.asarray(self.var2.t_dim_indices)
        diff = x[:, i1] - x[:, i2]
        return x, i1, i2, diff, np.sqrt((diff ** 2).sum(1))

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """log N(|t_1 - t_2| - observation; 0, sigma^2) at x = [var1 | var2] (reference :2724-2730, :2195-2201)."""
        return _range_log_pdf(self._residual(x)[-1], self._observation[0], self._sigma)

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d log_pdf / d[var1 | var2], float64 (reference :2732-2751, :2203-2223): along the line between the two ends,
        0 in a heading column, and the zero vector at a range of exactly 0 (the reference divides by it)."""
        x, i1, i2, diff, r = self._residual(x)
        g = _range_score(diff, r, self._observation[0], self._sigma)
        out = np.zeros_like(x)
        out[:, i1], out[:, i2] = g, -g
        return out

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d^2 log_pdf / d[var1 | var2]^2, [n, w, w] float64: the range block on the two ends' positions (negated across
        them), 0 in a heading row or column, and the zero block at a range of exactly 0."""
        x, i1, i2, diff, r = self._residual(x)
        h = _range_hess(diff, r, self._observation[0], self._sigma)
        out = np.zeros((x.shape[0], x.shape[1], x.shape[1]))
        out[:, i1[:, None], i1[None, :]], out[:, i2[:, None], i2[None, :]] = h, h
        out[:, i1[:, None], i2[None, :]], out[:, i2[:, None], i1[None, :]] = -h, -h
        return out

    def density_record(self) -> dict:
        return dict(code="RANGE", a=self.var1, b=self.var2, cand=[],
                    p=[float(self._observation[0]), 1.0 / self._sigma ** 2, _gaussian_log_norm(self._sigma ** 2)])

    def sample(self, var1=None, var2=None) -> np.ndarray:
        if var1 is None:
            if var2 is None:
                raise ValueError("Samples of at least one variable must be specified")
            return self.sample_var1_from_var2(var2)
        if var2 is None:
            return self.sample_var2_from_var1(var1)
        return self.sample_observations(var1, var2)

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        name_to_var = {v.name: v for v in variables}
        return cls(var1=name_to_var[tok[1]], var2=name_to_var[tok[2]], observation=float(tok[3]),
                   sigma=float(tok[4]))

    def __str__(self):
        return " ".join(["Factor", self.__class__.__name__, str(self.var1.name), str(self.var2.name),
                         str(self.observation[0]), str(self.sigma)])


# ---- ambiguous data association: one measurement, k candidate partners ----------------------------
class BinaryFactorMixture(LikelihoodFactor):
    """Mixture over `observed_vars` of binary factors of one class between the observer and each
    candidate (reference :3043-3181).  Simulation splits the sample batch among the hypotheses with a
    multinomial draw (rows of a sample batch are exchangeable)."""

    def __init__(self, observer_var: Variable, observed_vars: List[Variable], weights: np.ndarray,
                 binary_factor_class, obs_arr: List, sigma_arr: List):
        weights = np.asarray(weights, dtype=np.float64)
        assert np.all(weights > 0) and len(weights) == len(obs_arr) == len(sigma_arr) == len(observed_vars)
        self.observer_var = observer_var
        seen, uniq = set(), []
        for v in observed_vars:
            if v not in seen:
                seen.add(v)
                uniq.append(v)
        self.observed_vars = uniq
        self._vars = [observer_var] + self.observed_vars
        self.weights = weights / weights.sum()
        self.observations = obs_arr
        self.sigmas = sigma_arr
        self.components = [binary_factor_class(observer_var, v, obs_arr[i], sigma_arr[i])
                           for i, v in enumerate(observed_vars)]
        self.var2idx, off = {}, 0
        for v in self._vars:
            self.var2idx[v] = np.arange(off, off + v.dim)
            off += v.dim
        self.comp2idx = {c: np.concatenate((self.var2idx[c.var1], self.var2idx[c.var2])) for c in self.components}

    @property
    def vars(self):
        return self._vars

    @property
    def observation_var(self):
        return self.components[0].observation_var

    @property
    def measurement_dim(self):
        return self.observation_var.dim

    def _split(self, n):
        counts = np.random.multinomial(n, self.weights)
        bounds = np.concatenate(([0], np.cumsum(counts)))
        return [(int(bounds[i]), int(bounds[i + 1])) for i in range(len(self.components))]

    def sample_observations(self, var_samples) -> np.ndarray:
        """Simulated measurements given samples of every variable of the factor."""
        n = var_samples[self.observer_var].shape[0]
        out = np.zeros((n, self.measurement_dim))
        for (lo, hi), c in zip(self._split(n), self.components):
            if hi > lo:
                out[lo:hi] = c.sample(var1=var_samples[c.var1][lo:hi], var2=var_samples[c.var2][lo:hi])
        return out

    def pdf(self, x: np.ndarray) -> np.ndarray:
        return sum(c.pdf(x[:, self.comp2idx[c]]) * w for c, w in zip(self.components, self.weights))

    def _terms(self, x):
        """-> (x, the weighted component terms log w_k + log p_k(x), [k, n])."""
        x = _as_points(x, self.dim)
        return x, np.stack([c.log_pdf(x[:, self.comp2idx[c]]) + np.log(w) for c, w in zip(self.components, self.weights)])

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """log sum_k w_k p_k(x) by log-sum-exp: finite far from every component, where the reference's log of a sum of
        exps (:3126-3133) is -inf; equal to it wherever that is finite."""
        x, terms = self._terms(x)
        top = terms.max(0)
        return top + np.log(np.exp(terms - top).sum(0))

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d log_pdf / dx = sum_k r_k grad log p_k with r the softmax of the weighted component terms, shifted by their
        maximum like `log_pdf`: finite far from every component, where the reference (:3135-3156) divides by a sum of pdfs
        that has underflowed to 0.  A repeated candidate's contributions add into the same columns."""
        x, terms = self._terms(x)
        e = np.exp(terms - terms.max(0))
        r = e / e.sum(0)
        out = np.zeros_like(x)
        for k, c in enumerate(self.components):
            out[:, self.comp2idx[c]] += r[k][:, None] * c.grad_x_log_pdf(x[:, self.comp2idx[c]])
        return out

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d^2 log_pdf / dx^2 = sum_k r_k (H_k + g_k g_k') - g g' with the softmax weights r of `grad_x_log_pdf`, the
        components' gradients g_k and Hessians H_k in the factor's columns and g = sum_k r_k g_k, [n, w, w] float64.  Evaluated
        as sum_k r_k (H_k + (g_k - g)(g_k - g)'), the same matrix (sum_k r_k = 1) without the cancellation of |g|^2 where one
        component carries the weight."""
        x, terms = self._terms(x)
        e = np.exp(terms - terms.max(0))
        r = e / e.sum(0)
        out = np.zeros((x.shape[0], x.shape[1], x.shape[1]))
        gs = np.zeros((len(self.components),) + x.shape)
        for k, c in enumerate(self.components):
            idx = self.comp2idx[c]
            gs[k][:, idx] = c.grad_x_log_pdf(x[:, idx])
            out[:, idx[:, None], idx[None, :]] += r[k][:, None, None] * c.hess_x_log_pdf(x[:, idx])
        g = (r[:, :, None] * gs).sum(0)
        for k in range(len(self.components)):
            d = gs[k] - g
            out += r[k][:, None, None] * (d[:, :, None] * d[:, None, :])
        return out

    def density_record(self) -> dict:
        """A k-way range mixture: candidates may repeat (the null hypothesis: one landmark, two sigmas)."""
        if len(self.components) > 4:
            raise NotImplementedError("%s with %d components: the device table holds at most 4"
                                      % (self.__class__.__name__, len(self.components)))
        p = []
        for c, w in zip(self.components, self.weights):
            if not isinstance(c, SE2R2RangeGaussianLikelihoodFactor) or c.var1 != self.observer_var:
                raise NotImplementedError("%s over %s components has no device code (range components only)"
                                          % (self.__class__.__name__, c.__class__.__name__))
            r = c.density_record()["p"]
            p += [r[0], r[1], r[2] + float(np.log(w))]
        return dict(code="RANGE_MIX", a=self.observer_var, b=None, cand=[c.var2 for c in self.components], p=p)

    def posterior_weights(self, var2x) -> np.ndarray:
        """Re-weight the association hypotheses with posterior samples (reference :3158-3181)."""
        x = np.concatenate([var2x[v] for v in self.vars], axis=1)
        lik = np.array([c.pdf(x[:, self.comp2idx[c]]) * w for c, w in zip(self.components, self.weights)])
        tot = lik.sum(0)
        hw = np.full_like(lik, 0.5)
        ok = tot > 0
        hw[:, ok] = lik[:, ok] / tot[ok]
        return hw.sum(1) / hw.sum()


class AmbiguousDataAssociationFactor(BinaryFactorMixture, KWayFactor):
    """One measurement taken by `observer_var` of ONE of `observed_vars` (reference :3192-3298)."""

    def __init__(self, observer_var: Variable, observed_vars: List[Variable], weights: np.ndarray,
                 binary_factor_class, observation, sigma):
        k = len(observed_vars)
        assert k == len(weights)
        super().__init__(observer_var, observed_vars, weights, binary_factor_class, [observation] * k, [sigma] * k)

    @property
    def observation(self) -> np.ndarray:
        return self.components[0].observation

    @property
    def root_var(self) -> Variable:
        return self.observer_var

    @property
    def child_vars(self) -> List[Variable]:
        return self.observed_vars

    def sample_observer(self, var2sample) -> np.ndarray:
        """Samples of the observer given samples of all candidates."""
        n = var2sample[self.observed_vars[0]].shape[0]
        out = np.zeros((n, self.observer_var.dim))
        for (lo, hi), c in zip(self._split(n), self.components):
            if hi <= lo:
                continue
            if c.var1 == self.observer_var:
                out[lo:hi] = c.sample(var1=None, var2=var2sample[c.var2][lo:hi])
            elif c.var2 == self.observer_var:
                out[lo:hi] = c.sample(var1=var2sample[c.var1][lo:hi], var2=None)
            else:
                raise ValueError("None of the vars of component matches the observer var.")
        return out

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        name_to_var = {v.name: v for v in variables}
        i_obs, i_seen, i_w = tok.index("Observer") + 1, tok.index("Observed") + 1, tok.index("Weights") + 1
        i_cls, i_meas, i_sig = tok.index("Binary") + 1, tok.index("Observation") + 1, tok.index("Sigma") + 1
        observed = [name_to_var[t] for t in tok[i_seen:i_w - 1]]
        weights = np.array(tok[i_w:i_cls - 1], dtype=float)
        klass = _FACTOR_CLASSES[tok[i_cls]]
        if i_sig - i_meas - 1 != 1:
            raise NotImplementedError("vector-valued ambiguous measurements are not used by the shipped graphs")
        return cls(name_to_var[tok[i_obs]], observed, weights, klass, float(tok[i_meas]), float(tok[i_sig]))

    def __str__(self):
        return " ".join(["Factor", self.__class__.__name__, "Observer", str(self.observer_var.name), "Observed"] +
                        [str(v.name) for v in self.observed_vars] + ["Weights"] + [str(w) for w in self.weights] +
                        ["Binary", self.components[0].__class__.__name__, "Observation",
                         str(float(np.ravel(self.observation)[0])), "Sigma", str(self.components[0].sigma)])


_FACTOR_CLASSES = {c.__name__: c for c in (UnarySE2ApproximateGaussianPriorFactor,
                                           SE2RelativeGaussianLikelihoodFactor,
                                           SE2R2RangeGaussianLikelihoodFactor,
                                           AmbiguousDataAssociationFactor)}


# ---- the R2 family of the toy range-only examples (BASELINE config[2]; reference :362, :451/:2226, :912, :2026) ----
def _cov_of(covariance, precision):
    if covariance is not None:
        return np.array(covariance, dtype=np.float64)
    if precision is not None:
        return np.linalg.inv(np.array(precision, dtype=np.float64))
    raise ValueError("None of cov and info. were defined.")


def _mat2(tok, start):
    return np.array([[float(tok[start]), float(tok[start + 1])], [float(tok[start + 2]), float(tok[start + 3])]])


class UnaryR2GaussianPriorFactor(ExplicitPriorFactor, UnaryFactor):
    """x ~ N(mu, covariance) on the plane (reference :362-448)."""

    def __init__(self, var: Variable, mu: np.ndarray, covariance: np.ndarray = None, precision: np.ndarray = None):
        assert var.dim == 2
        self._vars = [var]
        self._mu = np.array(mu, dtype=np.float64).ravel()
        self._covariance = _cov_of(covariance, precision)
        self._chol = np.linalg.cholesky(self._covariance)

    @property
    def vars(self):
        return self._vars

    @property
    def mu(self):
        return self._mu

    @property
    def observation(self):
        return self._mu

    @property
    def covariance(self):
        return self._covariance

    @property
    def is_gaussian(self):
        return True

    def sample(self, num_samples: int, **kwargs) -> np.ndarray:
        return self._mu + _gaussian_noise(self._chol, num_samples)

    def _residual(self, x):
        return _as_points(x, 2) - self._mu

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """log N(x; mu, covariance) (reference :373: the distribution's own log_pdf)."""
        return _gaussian_log_norm(self._covariance) - 0.5 * _quad_form(self._residual(x), np.linalg.inv(self._covariance))

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """-precision (x - mu), [n, 2] float64."""
        P = np.linalg.inv(self._covariance)
        return -self._residual(x) @ (0.5 * (P + P.T))

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """-precision at every point, [n, 2, 2] float64."""
        P = np.linalg.inv(self._covariance)
        return np.broadcast_to(-0.5 * (P + P.T), (_as_points(x, 2).shape[0], 2, 2)).copy()

    def density_record(self) -> dict:
        return dict(code="PRIOR_R2", a=self.var, b=None, cand=[],
                    p=[float(self._mu[0]), float(self._mu[1])] + _sym_upper(np.linalg.inv(self._covariance)) +
                      [_gaussian_log_norm(self._covariance)])

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        if tok[4] not in ("covariance", "precision"):
            raise ValueError("Must specify either covariance or precision")
        var = {v.name: v for v in variables}[tok[1]]
        return cls(var=var, mu=np.array([float(tok[2]), float(tok[3])]), **{tok[4]: _mat2(tok, 5)})

    def __str__(self):
        c = self._covariance
        return " ".join(["Factor", self.__class__.__name__, str(self.var.name), str(self._mu[0]), str(self._mu[1]),
                         "covariance", str(c[0, 0]), str(c[0, 1]), str(c[1, 0]), str(c[1, 1])])


class UnaryR2RangeGaussianPriorFactor(ExplicitPriorFactor, UnaryFactor):
    """x on a ring around `center`: radius ~ N(mu, sigma^2), uniform bearing (reference :451-533, :2226-2308;
    draws: src/stats/Distributions.py:125-130)."""

    def __init__(self, var: Variable, center: np.ndarray, mu: float, sigma: float):
        assert var.dim == 2
        self._vars = [var]
        self._center = np.array(center, dtype=np.float64).ravel()
        self._mu, self._sigma = float(mu), float(sigma)

    @property
    def vars(self):
        return self._vars

    @property
    def center(self):
        return self._center

    @property
    def mu(self):
        return self._mu

    @property
    def observation(self):
        return self._mu

    @property
    def sigma(self):
        return self._sigma

    def sample(self, num_samples: int, **kwargs) -> np.ndarray:
        r = self._mu + self._sigma * np.random.standard_normal(num_samples)
        phi = np.random.uniform(-np.pi, np.pi, num_samples)
        return self._center + np.stack([r * np.cos(phi), r * np.sin(phi)], 1)

    def _residual(self, x):
        diff = _as_points(x, 2) - self._center[None, :]
        return diff, np.sqrt((diff ** 2).sum(1))

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """log N(|x - center| - mu; 0, sigma^2): the range likelihood (reference :2195-2201) with one end at the centre,
        i.e. the density of the radius `sample` draws (see the module docstring on the reference's own body)."""
        return _range_log_pdf(self._residual(x)[-1], self._mu, self._sigma)

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d log_pdf / dx, [n, 2] float64: the range term's derivative with one end at the centre; 0 at the centre itself."""
        return _range_score(*self._residual(x), self._mu, self._sigma)

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d^2 log_pdf / dx^2, [n, 2, 2] float64: the range block with one end at the centre; 0 at the centre itself."""
        return _range_hess(*self._residual(x), self._mu, self._sigma)

    def density_record(self) -> dict:
        return dict(code="PRIOR_R2_RANGE", a=self.var, b=None, cand=[],
                    p=[float(self._center[0]), float(self._center[1]), self._mu, 1.0 / self._sigma ** 2,
                       _gaussian_log_norm(self._sigma ** 2)])

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        var = {v.name: v for v in variables}[tok[1]]
        if tok[2] == "center":                      # the form `__str__` writes (reference :486-491)
            return cls(var, np.array([float(tok[3]), float(tok[4])]), float(tok[6]), float(tok[8]))
        return cls(var, np.array([float(tok[2]), float(tok[3])]), float(tok[4]), float(tok[5]))   # reference :500-505

    def __str__(self):
        return " ".join(["Factor", self.__class__.__name__, str(self.var.name), "center", str(self._center[0]),
                         str(self._center[1]), "mu", str(self._mu), "sigma", str(self._sigma)])


class R2RelativeGaussianLikelihoodFactor(LikelihoodFactor, BinaryFactor, OdomFactor):
    """var2 - var1 = observation + N(0, covariance) (reference :912-1092)."""
    measurement_dim = 2
    measurement_type = R2Variable

    def __init__(self, var1: Variable, var2: Variable, observation: np.ndarray, covariance: np.ndarray = None,
                 precision: np.ndarray = None):
        if var1.dim != var2.dim:
            raise ValueError("The two variables must have the same dimensionality")
        if len(observation) != var1.dim:
            raise ValueError("The observation must have the same dimensionality as the two variables")
        self._vars = [var1, var2]
        self._observation = np.array(observation, dtype=np.float64).ravel()
        self._covariance = _cov_of(covariance, precision)
        self._chol = np.linalg.cholesky(self._covariance)
        self._observation_var = R2Variable(name="O" + str(var1.name) + str(var2.name),
                                           variable_type=VariableType.Measurement)

    @property
    def vars(self):
        return self._vars

    @property
    def observation(self):
        return self._observation

    @property
    def observation_var(self):
        return self._observation_var

    @property
    def circular_dim_list(self):
        return self._observation_var.circular_dim_list

    @property
    def covariance(self):
        return self._covariance

    @property
    def is_gaussian(self):
        return True

    def sample(self, var1: np.ndarray = None, var2: np.ndarray = None) -> np.ndarray:
        """var2 given -> var1 samples; var1 given -> var2 samples; both -> simulated observations (reference :998-1030)."""
        if var1 is None:
            if var2 is None:
                raise ValueError("Samples of at least one variable must be specified")
            return var2 - _gaussian_noise(self._chol, var2.shape[0]) - self._observation
        if var2 is None:
            return var1 + _gaussian_noise(self._chol, var1.shape[0]) + self._observation
        if var1.shape != var2.shape or var1.shape[1] != 2:
            raise ValueError("Dimensionality of variable 1 or variable 2 is wrong")
        return var2 - var1 + _gaussian_noise(self._chol, var1.shape[0])

    def _residual(self, x):
        x = _as_points(x, 4)
        return x[:, 2:] - x[:, :2] - self._observation

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        """log N(var2 - var1 - observation; 0, covariance) at x = [var1 | var2] (reference :1070-1074)."""
        return _gaussian_log_norm(self._covariance) - 0.5 * _quad_form(self._residual(x), np.linalg.inv(self._covariance))

    def grad_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d log_pdf / d[var1 | var2], [n, 4] float64: +-precision (var2 - var1 - observation)."""
        P = np.linalg.inv(self._covariance)
        g = -self._residual(x) @ (0.5 * (P + P.T))
        return np.concatenate([-g, g], 1)

    def hess_x_log_pdf(self, x: np.ndarray) -> np.ndarray:
        """d^2 log_pdf / d[var1 | var2]^2, [n, 4, 4] float64: -precision on both diagonal blocks, +precision across."""
        P = np.linalg.inv(self._covariance)
        P = 0.5 * (P + P.T)
        return np.broadcast_to(np.block([[-P, P], [P, -P]]), (_as_points(x, 4).shape[0], 4, 4)).copy()

    def density_record(self) -> dict:
        return dict(code="REL_R2", a=self.var1, b=self.var2, cand=[],
                    p=[float(self._observation[0]), float(self._observation[1])] +
                      _sym_upper(np.linalg.inv(self._covariance)) + [_gaussian_log_norm(self._covariance)])

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != cls.__name__:
            raise ValueError("The factor name is incorrect")
        name_to_var = {v.name: v for v in variables}
        return cls(var1=name_to_var[tok[1]], var2=name_to_var[tok[2]], observation=np.array([float(tok[3]), float(tok[4])]),
                   **{tok[5]: _mat2(tok, 6)})

    def __str__(self):
        c = self._covariance
        return " ".join(["Factor", self.__class__.__name__, str(self.var1.name), str(self.var2.name),
                         str(self._observation[0]), str(self._observation[1]), "covariance",
                         str(c[0, 0]), str(c[0, 1]), str(c[1, 0]), str(c[1, 1])])


class R2RangeGaussianLikelihoodFactor(SE2R2RangeGaussianLikelihoodFactor):
    """|var2 - var1| = observation + N(0, sigma^2) between two points of the plane (reference :2026-2223): the same
    ring / simulated-range draws as the pose-landmark range factor (both variables' translation indices are 0, 1)."""

    def __init__(self, var1: Variable, var2: Variable, observation: Union[np.ndarray, float], sigma: float = 1.0):
        if var1.dim != 2 or var2.dim != 2:
            raise ValueError("R2RangeGaussianLikelihoodFactor connects two R2 variables")
        super().__init__(var1, var2, observation, sigma)


_FACTOR_CLASSES.update({c.__name__: c for c in (UnaryR2GaussianPriorFactor, UnaryR2RangeGaussianPriorFactor,
                                                R2RelativeGaussianLikelihoodFactor, R2RangeGaussianLikelihoodFactor)})


# ---- a binary factor that may be an outlier (reference :3300-3462) -------------------------------------
class _BinaryFactorWithNullHypo(BinaryFactorMixture, BinaryFactorWithNullHypo):
    """Two hypotheses about ONE measurement between var1 and var2: the regular factor (sigma) and a "null" one that
    keeps the measurement but inflates its noise by `null_sigma_scale`; `weights` = (regular, null)."""

    def __init__(self, var1: Variable, var2: Variable, weights: np.ndarray, binary_factor_class, observation, sigma,
                 null_sigma_scale: float = 10.0):
        assert len(weights) == 2
        self.null_sigma_scale = float(null_sigma_scale)
        super().__init__(var1, [var2, var2], weights, binary_factor_class, [observation] * 2,
                         [sigma, sigma * self.null_sigma_scale])

    @property
    def var1(self) -> Variable:
        return self.observer_var

    @property
    def var2(self) -> Variable:
        return self.observed_vars[0]

    @property
    def observation(self) -> np.ndarray:
        return self.components[0].observation

    def _mix(self, n, draw):
        out = None
        for (lo, hi), c in zip(self._split(n), self.components):
            if hi > lo:
                part = draw(c, lo, hi)
                if out is None:
                    out = np.zeros((n, part.shape[1]))
                out[lo:hi] = part
        return out

    def sample(self, var1=None, var2=None) -> np.ndarray:
        """var2 given -> var1 samples; var1 given -> var2 samples; both -> simulated observations."""
        if var1 is None:
            if var2 is None:
                raise ValueError("Samples of at least one variable must be specified")
            return self._mix(var2.shape[0], lambda c, lo, hi: c.sample(var1=None, var2=var2[lo:hi]))
        if var2 is None:
            return self._mix(var1.shape[0], lambda c, lo, hi: c.sample(var1=var1[lo:hi], var2=None))
        return self._mix(var1.shape[0], lambda c, lo, hi: c.sample(var1=var1[lo:hi], var2=var2[lo:hi]))

    @classmethod
    def construct_from_text(cls, line: str, variables):
        tok = line.strip().split()
        if tok[0] != "BinaryFactorWithNullHypo":
            raise ValueError("The factor name is incorrect")
        name_to_var = {v.name: v for v in variables}
        i_obsr, i_obsd, i_w = tok.index("Observer") + 1, tok.index("Observed") + 1, tok.index("Weights") + 1
        i_cls, i_obs, i_sig = tok.index("Binary") + 1, tok.index("Observation") + 1, tok.index("Sigma") + 1
        i_null = tok.index("NullSigmaScale") + 1
        klass = _FACTOR_CLASSES[tok[i_cls]]
        if klass.measurement_dim != 1:
            raise NotImplementedError("null-hypothesis factors are rebuilt for scalar measurements (range factors)")
        weights = np.array(tok[i_w:i_cls - 1], dtype=float)
        return cls(name_to_var[tok[i_obsr]], name_to_var[tok[i_obsd]], weights, klass, float(tok[i_obs]),
                   float(tok[i_sig]), float(tok[i_null]))

    def __str__(self):
        return " ".join(["Factor", "BinaryFactorWithNullHypo", "Observer", str(self.var1.name), "Observed",
                         str(self.var2.name), str(self.var2.name), "Weights"] + [str(w) for w in self.weights] +
                        ["Binary", self.components[0].__class__.__name__, "Observation",
                         str(float(np.ravel(self.observation)[0])), "Sigma", str(self.components[0].sigma),
                         "NullSigmaScale", str(self.null_sigma_scale)])


_BinaryFactorWithNullHypo.__name__ = "BinaryFactorWithNullHypo"
_BinaryFactorWithNullHypo.__qualname__ = "BinaryFactorWithNullHypo"
BinaryFactorWithNullHypo = _BinaryFactorWithNullHypo           # the name the reference exports (isinstance dispatch keeps working)
_FACTOR_CLASSES["BinaryFactorWithNullHypo"] = BinaryFactorWithNullHypo
