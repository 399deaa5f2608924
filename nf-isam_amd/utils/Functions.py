"""utils.Functions — the helpers of the reference's `utils/Functions.py` that this solver uses: angle wrapping, which sits on
the hot path (reference: src/utils/Functions.py:20-21), and the point-set alignment its trajectory plots grade with
(reference: :53-71)."""
import numpy as np

_TWO_PI = 2 * np.pi


def theta_to_pipi(theta):
    """Wrap angles into [-pi, pi).  Works on numpy arrays and torch tensors alike."""
    return (theta + np.pi) % _TWO_PI - np.pi


def kabsch_umeyama(A, B, reflect=False):
    """The similarity transform that brings the points B [n, m] onto A [n, m] in the least-squares sense of Umeyama (IEEE
    PAMI 13(4), 1991): -> (R [m, m], c, t [m]) with A ~ c R B + t.  The reference's surface function (src/utils/Functions.py:53-71)
    for any dimension m.

    With a', b' the two sets about their means and H = a'^T b' / n = U diag(D) V^T, the rotation is R = U S V^T where
    S = diag(1, ..., 1, d) and d = sign(det U det V^T) keeps R proper (det R = +1).  reflect=True takes S = I instead: the best
    orthogonal map, a reflection where that fits better.

    The scale keeps the reference's rule, c = Var_A / tr(diag(D) S) with Var_A = mean |a'|^2.  That is sum |a'|^2 / g for
    g = n tr(diag(D) S), NOT the least-squares scale of Umeyama's eq. (42), g / sum |b'|^2, which the device evaluator's
    "similarity" mode uses: the two agree exactly when A is an exact similarity of B, and differ by the factor
    sum |a'|^2 sum |b'|^2 / g^2 >= 1 otherwise.  t is formed with that c."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or A.shape != B.shape or A.shape[0] < 1:
        raise ValueError("A and B must be two [n, m] point sets of one shape, got %s and %s" % (A.shape, B.shape))
    n, m = A.shape
    mean_a, mean_b = A.mean(axis=0), B.mean(axis=0)
    da, db = A - mean_a, B - mean_b
    var_a = np.sum(da * da) / n
    U, D, Vt = np.linalg.svd(da.T @ db / n)
    S = np.ones(m)
    if not reflect and np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[-1] = -1.0
    R = (U * S) @ Vt
    c = var_a / np.sum(D * S)
    t = mean_a - c * R @ mean_b
    return R, c, t
