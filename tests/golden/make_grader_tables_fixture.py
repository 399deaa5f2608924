#!/usr/bin/env python
"""tests/golden/grader_tables.npz: the tables the solver's two-sample graders (`posterior_mmd`, `posterior_mmd_test`,
`posterior_transport`, the reference branch of `posterior_information`) hand to their launches, as the code computed them at
the commit BEFORE the graders shared one reference front.  The committed file is the fixture: a rerun at a later commit
stores that commit's tables and proves nothing about the earlier ones.

What is stored is `tests/test_posterior_evaluation_cpu.py::grader_tables()`, which the test of the same file recomputes and
compares array by array.  No GPU, no reference checkout; seconds.

    python tests/golden/make_grader_tables_fixture.py       # rewrites tests/golden/grader_tables.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the source roots on sys.path)
from test_posterior_evaluation_cpu import grader_tables  # noqa: E402


def main():
    out = grader_tables()
    path = os.path.join(HERE, "grader_tables.npz")
    np.savez_compressed(path, **out)
    print(path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
