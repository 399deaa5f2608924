#!/usr/bin/env python
"""tests/golden/trajectory_error.npz from the REFERENCE ITSELF (build container only: needs /root/reference; nothing of it travels).

A few fixed float32 point sets (an estimate B, a float64 truth A) and what the reference's own `kabsch_umeyama`
(/root/reference/src/utils/Functions.py:53-71) returns for them -- R, c, t -- with the RMSE its Plaza scripts then report,
sqrt(mean |A - (c R B + t)|^2), computed from the float32 points cast to float64.  The reference's module imports pandas
(present here) and its own packages; what those import besides is stubbed the way make_sample_summary_fixture.py does it.

    python tests/golden/make_trajectory_error_fixture.py          # rewrites tests/golden/trajectory_error.npz (tens of KB)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_pipeline_fixture import REF, write_stubs  # noqa: E402

# (name, points, offset of the truth, extent of the path, rotation, scale, translation, noise)
CASES = [
    ("two", 2, (1.0, -2.0), 5.0, 0.7, 1.0, (0.5, 0.25), 0.05),
    ("three", 3, (0.0, 0.0), 5.0, -2.1, 1.3, (-4.0, 9.0), 0.05),
    ("forty", 40, (3.0, -7.0), 30.0, 0.4, 0.9, (12.0, 3.0), 0.2),
    ("far", 40, (100.0, 100.0), 20.0, 0.05, 1.0, (0.3, -0.2), 0.01),            # 100 m offsets, centimetre noise
    ("nearly_pi", 40, (3.0, -7.0), 30.0, np.pi - 1e-3, 1.0, (1.0, 1.0), 0.1),    # rotated by nearly pi
]


def main():
    tmp = tempfile.mkdtemp(prefix="nfisam_ref_")
    write_stubs(os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(REF, "src"))
    sys.dont_write_bytecode = True
    import utils.Functions as RF
    rng = np.random.RandomState(20241021)
    out = {"names": np.array([c[0] for c in CASES])}
    for name, P, offset, extent, rot, scale, shift, noise in CASES:
        # a wandering path as the truth; the estimate is the truth moved by the INVERSE similarity, plus noise
        A = np.cumsum(rng.standard_normal((P, 2)), axis=0) * extent / np.sqrt(P) + np.asarray(offset)
        R = np.array([[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]])
        B = ((A - np.asarray(shift)) @ R) / scale + rng.standard_normal((P, 2)) * noise
        B = B.astype(np.float32)
        B64 = B.astype(np.float64)
        Rr, c, t = RF.kabsch_umeyama(A, B64)
        rmse = np.sqrt(np.mean(np.sum((A - (c * B64 @ Rr.T + t)) ** 2, axis=1)))
        out["A_" + name], out["B_" + name] = A, B
        out["R_" + name], out["c_" + name], out["t_" + name] = np.asarray(Rr), np.float64(c), np.asarray(t)
        out["rmse_" + name] = np.float64(rmse)
        print(name, P, float(c), np.asarray(t), float(rmse))
    path = os.path.join(HERE, "trajectory_error.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
