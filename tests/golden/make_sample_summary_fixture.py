#!/usr/bin/env python
"""tests/golden/sample_summary.npz from the REFERENCE ITSELF (build container only: needs /root/reference; nothing of it travels).

A few fixed float32 sample sets over poses and landmarks -- one of them with a heading whose mass straddles +-pi -- and what the
reference's own `sample_mean`, `translation_distance`, `geodesic_distance` and `rmse`
(/root/reference/src/utils/Statistics.py:142-214) return for them, computed from the float32 points cast to float64.  The
reference's module imports TransportMaps at module level (absent here, unused by these functions): stubbed the way
make_pipeline_fixture.py does it.  Variables travel as their kinds ("SE2" / "R2"), one per variable, in column order.

    python tests/golden/make_sample_summary_fixture.py          # rewrites tests/golden/sample_summary.npz (tens of KB)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_pipeline_fixture import REF, write_stubs  # noqa: E402

# (points, kinds, centre of every variable, spread of its xy, spread of its heading)
CASES = [
    (200, ["SE2", "SE2", "R2"], [(1.0, -2.0, 0.3), (105.0, 48.0, 3.0), (-7.5, 12.25)], 0.4, 0.25),     # heading 2 straddles +-pi
    (257, ["R2", "R2", "R2", "R2"], [(0.0, 0.0), (30.0, -40.0), (100.0, 100.0), (-3.0, 2.0)], 0.01, 0.0),
    (64, ["SE2", "R2", "SE2", "SE2"], [(3.0, 3.0, -3.1), (8.0, -1.0), (50.0, 60.0, 1.5), (-20.0, 5.0, -0.7)], 1.5, 0.6),
    (33, ["SE2"], [(0.5, 0.25, 3.14)], 0.05, 0.02),
]


def main():
    tmp = tempfile.mkdtemp(prefix="nfisam_ref_")
    write_stubs(os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(REF, "src"))
    sys.dont_write_bytecode = True
    import sklearn.metrics  # noqa: F401  (the reference's module says `import sklearn`)
    import utils.Statistics as RS
    from slam.Variables import R2Variable, SE2Variable
    rng = np.random.RandomState(20241018)
    out = {"n_cases": np.int64(len(CASES))}
    for k, (n, kinds, centres, s_xy, s_th) in enumerate(CASES):
        variables = [SE2Variable("X%d" % i) if kind == "SE2" else R2Variable("L%d" % i) for i, kind in enumerate(kinds)]
        parts = []
        for kind, c in zip(kinds, centres):
            xy = rng.standard_normal((n, 2)) * s_xy + np.asarray(c[:2])
            if kind == "SE2":
                th = (rng.standard_normal((n, 1)) * s_th + c[2] + np.pi) % (2.0 * np.pi) - np.pi
                xy = np.hstack([xy, th])
            parts.append(xy)
        x = np.hstack(parts).astype(np.float32)
        x64 = x.astype(np.float64)
        means, var2mean = RS.sample_mean(x64, variables)
        # a second assignment to measure distances to: the centres, nudged
        other, at = {}, 0
        for v, c in zip(variables, centres):
            other[v] = np.asarray(c, dtype=np.float64) + rng.standard_normal(len(c)) * 0.1
            at += v.dim
        out["samples%d" % k] = x
        out["kinds%d" % k] = np.array(kinds)
        out["means%d" % k] = np.asarray(means, dtype=np.float64)
        out["other%d" % k] = np.concatenate([other[v] for v in variables])
        out["translation%d" % k] = np.float64(RS.translation_distance(var2mean, other))
        out["geodesic%d" % k] = np.float64(RS.geodesic_distance(var2mean, other))
        shifted = (x64[::-1] * 1.01 + 0.125)
        out["rmse_other%d" % k] = shifted
        out["rmse%d" % k] = np.float64(RS.rmse(x64, shifted))
        print(k, n, kinds, float(out["translation%d" % k]), float(out["geodesic%d" % k]), float(out["rmse%d" % k]))
    path = os.path.join(HERE, "sample_summary.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
