#!/usr/bin/env python
"""tests/golden/sample_mmd.npz from the REFERENCE ITSELF (build container only: needs /root/reference; nothing of it travels).

Six (m, n, d, sigma) cases of two float32 sample sets and the values the reference's own `MMDb` and `MMDu2`
(/root/reference/src/utils/Statistics.py:46-84, sklearn's pairwise distances) return for them -- computed from the float32
points cast to float64, which is what the device entry evaluates.  The reference's module imports TransportMaps at module
level (absent here, unused by these two functions): stubbed the way make_pipeline_fixture.py does it.

    python tests/golden/make_sample_mmd_fixture.py          # rewrites tests/golden/sample_mmd.npz (~60 KB)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_pipeline_fixture import REF, write_stubs  # noqa: E402

# (m, n, d, sigma, offset of the second set): odd sizes, sizes around the device tile of 64, column counts around its chunk of 16
CASES = [(37, 53, 1, 1.0, 0.5), (64, 65, 2, float(np.sqrt(2.0)), 0.3), (130, 63, 3, 0.7, 0.4), (100, 200, 16, 4.0, 0.25),
         (129, 70, 17, float(np.sqrt(17.0)), 0.2), (80, 90, 40, float(np.sqrt(40.0)), 0.15)]


def main():
    tmp = tempfile.mkdtemp(prefix="nfisam_ref_")
    write_stubs(os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(tmp, "stubs"))
    sys.path.insert(0, os.path.join(REF, "src"))
    sys.dont_write_bytecode = True
    import sklearn.metrics  # noqa: F401  (the reference says `import sklearn` and uses sklearn.metrics)
    import utils.Statistics as RS
    rng = np.random.RandomState(20240610)
    out = {"cases": np.array([c[:4] for c in CASES], dtype=np.float64)}
    for k, (m, n, d, sigma, shift) in enumerate(CASES):
        x = (rng.standard_normal((m, d)) * 1.5 + 3.0).astype(np.float32)
        y = (rng.standard_normal((n, d)) * 1.2 + 3.0 + shift).astype(np.float32)
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        out["x%d" % k], out["y%d" % k] = x, y
        out["MMDb%d" % k] = np.float64(RS.MMDb(x64, y64, sigma))
        out["MMDu2%d" % k] = np.float64(RS.MMDu2(x64, y64, sigma))
        print(k, (m, n, d, sigma), float(out["MMDb%d" % k]), float(out["MMDu2%d" % k]))
    path = os.path.join(HERE, "sample_mmd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
