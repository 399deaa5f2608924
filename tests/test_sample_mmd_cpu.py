"""The two-sample MMD without a GPU: the surface of the device entry (header, exports, struct size), the refusals of the
binding and of `NFiSAM.posterior_mmd` before anything is launched, and the estimator algebra of `utils.Statistics`:
`mmd_from_sums` of kernel sums (float64 numpy, direct differences) against `MMDb`, `MMDu2` and `mmd` on the same arrays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- shared with tests/test_sample_mmd_gpu.py -----------------------------------------------------------------------------
def wrap_pi(t):
    return (t + np.pi) % (2.0 * np.pi) - np.pi


def oracle_sums(x, y, xcols, ycols, inv_two_sigma2, scale=None, wrap=None):
    """{Sxx, Syy, Sxy} of one block in float64 by direct differences, broadcast as (m, n, d), at the float32 points."""
    x, y = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
    out = []
    for a, ac, b, bc in ((x, xcols, x, xcols), (y, ycols, y, ycols), (x, xcols, y, ycols)):
        diff = a[:, None, ac] - b[None, :, bc]
        if wrap is not None:
            diff = np.where(np.asarray(wrap, dtype=bool)[None, None, :], wrap_pi(diff), diff)
        if scale is not None:
            diff = diff * np.asarray(scale, dtype=np.float64)[None, None, :]
        out.append(np.exp(-inv_two_sigma2 * (diff * diff).sum(-1)).sum())
    return np.array(out)


class Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_and_the_abi_version_stays():
    nh.build()
    lib = nh.lib()
    for name in ("nfisam_sample_mmd", "nfisam_sample_mmd_scratch_count"):
        assert name in nh.EXPORTS and hasattr(lib, name), name
    assert lib.nfisam_abi_version() == 1600
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    assert "int nfisam_sample_mmd(" in hdr and "size_t nfisam_sample_mmd_scratch_count(" in hdr
    assert callable(nh.mmd_sums) and callable(nh.mmd_sums_t) and callable(ST.mmd_blocks)


def test_struct_size_is_16_and_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfisam_hip.h"\nint main(void) { '
                   'printf("%zu %zu %zu\\n", sizeof(nfisam_mmd_block), offsetof(nfisam_mmd_block, d), '
                   'offsetof(nfisam_mmd_block, inv_two_sigma2)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [16, 4, 8]
    assert sizes == [C.sizeof(nh.MmdBlock), nh.MmdBlock.d.offset, nh.MmdBlock.inv_two_sigma2.offset]
    assert nh.MMD_BLOCK_DTYPE.itemsize == 16
    assert [nh.MMD_BLOCK_DTYPE.fields[k][1] for k in ("col_off", "d", "inv_two_sigma2")] == [0, 4, 8]


def test_scratch_count_and_host_side_refusals_of_the_c_entry():
    """The count is one double per (block, 64 x 64 tile of any of the three sums); the entry refuses bad arguments on the
    host, before it touches the device (the pointers below are never dereferenced: they are not device memory)."""
    nh.build()
    lib = nh.lib()
    count = lib.nfisam_sample_mmd_scratch_count
    assert count(1, 1, 1) == 3 and count(64, 64, 2) == 6 and count(65, 64, 1) == 3 + 1 + 2
    assert count(130, 200, 7) == 7 * (6 + 10 + 12)
    assert count(0, 5, 1) == 0 and count(5, 0, 1) == 0 and count(5, 5, 0) == 0
    blocks = nh.pack_mmd_blocks([2], [1.0])
    fake = C.c_void_p(4096)

    def call(Xt=fake, m=5, n=5, blk=blocks, blk_dev=fake, nb=1, sums=fake):
        return lib.nfisam_sample_mmd(Xt, 4, m, fake, 4, n, blk.ctypes.data_as(C.c_void_p), blk_dev, nb, fake, fake, 2, None, None,
                                     sums, fake, None)
    assert call(Xt=None) == nh.ERR_ARG and call(sums=None) == nh.ERR_ARG and call(blk_dev=None) == nh.ERR_ARG
    assert call(m=0) == nh.ERR_ARG and call(n=0) == nh.ERR_ARG and call(nb=0) == nh.ERR_ARG and call(nb=65536) == nh.ERR_ARG
    for d, v in ((0, 0.5), (2, 0.0), (2, -1.0), (2, np.inf), (2, np.nan)):
        bad = blocks.copy()
        bad["d"], bad["inv_two_sigma2"] = d, v
        assert call(blk=bad) == nh.ERR_ARG, (d, v)


def test_check_mmd_blocks_refuses_bad_offsets_and_rows():
    t = nh.pack_mmd_blocks([2, 3], [1.0, 2.0])
    assert list(t["col_off"]) == [0, 2] and list(t["d"]) == [2, 3] and np.allclose(t["inv_two_sigma2"], [0.5, 0.125])
    xc, yc = [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]
    nh.check_mmd_blocks(t, xc, yc, 5, 5)
    nh.check_mmd_blocks(t, xc, yc, 5, 5, scale=np.ones(5), wrap=np.zeros(5, dtype=np.uint8))
    for field, value, match in (("col_off", 3, "leave"), ("col_off", -1, "leave"), ("d", 0, "leave"), ("d", 4, "leave"),
                                ("inv_two_sigma2", 0.0, "positive"), ("inv_two_sigma2", np.nan, "positive"),
                                ("inv_two_sigma2", np.inf, "positive")):
        bad = t.copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match=match):
            nh.check_mmd_blocks(bad, xc, yc, 5, 5)
    with pytest.raises(ValueError, match="xcols"):
        nh.check_mmd_blocks(t, xc, yc, 4, 5)
    with pytest.raises(ValueError, match="ycols"):
        nh.check_mmd_blocks(t, xc, yc, 5, 4)
    with pytest.raises(ValueError, match="xcols"):
        nh.check_mmd_blocks(t, [0, 1, -1, 3, 4], yc, 5, 5)
    with pytest.raises(ValueError, match="same length"):
        nh.check_mmd_blocks(t, xc, yc[:4], 5, 5)
    with pytest.raises(ValueError, match="scale"):
        nh.check_mmd_blocks(t, xc, yc, 5, 5, scale=np.ones(4))
    with pytest.raises(ValueError, match="wrap"):
        nh.check_mmd_blocks(t, xc, yc, 5, 5, wrap=np.ones(6))
    with pytest.raises(ValueError, match="MMD_BLOCK_DTYPE"):
        nh.check_mmd_blocks(np.zeros(2), xc, yc, 5, 5)
    with pytest.raises(ValueError, match="blocks"):
        nh.check_mmd_blocks(t[:0], xc, yc, 5, 5)


def test_mmd_sums_refuses_cpu_tensors_and_bad_tables_before_any_launch(monkeypatch):
    refuse = Refuse()
    monkeypatch.setattr(nh, "upload", refuse)
    t = nh.pack_mmd_blocks([2], [1.0])
    X, Y = torch.zeros(5, 3), torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.mmd_sums(X, Y, t, [0, 1], [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.mmd_sums(X.numpy(), Y.numpy(), t, [0, 1], [0, 1], device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.mmd_sums_t(X.t().contiguous(), Y.t().contiguous(), t, [0, 1], [0, 1])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ST.mmd_blocks(X, Y, [[0, 1]])
    with pytest.raises(ValueError, match="xcols"):                     # refused before the device is asked for
        nh.mmd_sums(X.numpy(), Y.numpy(), t, [0, 3], [0, 1], device="cuda")
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        nh.mmd_sums(np.zeros(5, dtype=np.float32), Y.numpy(), t, [0, 1], [0, 1], device="cuda")
    assert refuse.calls == 0


# ---- the estimator algebra --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,d", [(2, 2, 1), (7, 5, 2), (30, 41, 3), (33, 20, 6)])
def test_estimators_from_sums_equal_the_statistics_functions(m, n, d):
    rng = np.random.RandomState(m * 100 + n)
    x = rng.standard_normal((m, d)).astype(np.float32).astype(np.float64)
    y = (rng.standard_normal((n, d)) * 1.3 + 0.4).astype(np.float32).astype(np.float64)
    cols = list(range(d))
    for sigma in (np.sqrt(d), 0.6):
        sums = oracle_sums(x, y, cols, cols, 1.0 / (2.0 * sigma ** 2))
        assert np.isclose(ST.mmd_from_sums(sums, m, n, "MMDb")[0], ST.MMDb(x, y, sigma), rtol=1e-9, atol=1e-12)
        assert np.isclose(ST.mmd_from_sums(sums, m, n, "MMDu2")[0], ST.MMDu2(x, y, sigma), rtol=1e-9, atol=1e-12)
        ref = ST.mmd(x, y, sigma ** 2)[0]
        got = ST.mmd_from_sums(sums, m, n, "mmd")[0]
        assert (np.isnan(ref) and np.isnan(got)) or np.isclose(got, ref, rtol=1e-8, atol=1e-12), (got, ref)
    # several blocks at once, the unbiased combination negative for a set against itself -> the reference's NaN
    same = oracle_sums(x, x, cols, cols, 0.5)
    other = oracle_sums(x, x[::-1] + 0.25, cols, cols, 0.5)
    u2 = ST.mmd_from_sums(np.stack([same, other]), m, m, "MMDu2")
    assert u2.shape == (2,) and u2[0] < 0 and u2[1] == ST.mmd_from_sums(other, m, m, "MMDu2")[0]
    assert np.isnan(ST.mmd_from_sums(same, m, m, "mmd")[0])
    assert ST.mmd_from_sums(same, m, m, "MMDb")[0] == 0.0


def test_estimator_refusals():
    sums = np.array([[1.0, 1.0, 1.0]])
    assert ST.mmd_from_sums(sums, 1, 1, "MMDb")[0] == 0.0
    for est in ("MMDu2", "mmd"):
        with pytest.raises(ValueError, match="two points"):
            ST.mmd_from_sums(sums, 1, 5, est)
        with pytest.raises(ValueError, match="two points"):
            ST.mmd_from_sums(sums, 5, 1, est)
        with pytest.raises(ValueError, match="at least 2"):
            ST.mmd_blocks(np.zeros((1, 2)), np.zeros((5, 2)), [[0, 1]], estimator=est)
    with pytest.raises(ValueError, match="estimator"):
        ST.mmd_from_sums(sums, 5, 5, "mmdb")
    with pytest.raises(ValueError, match="estimator"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [[0, 1]], estimator="MMD")
    with pytest.raises(ValueError, match="outside"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [[0, 2]])
    with pytest.raises(ValueError, match="outside"):
        ST.mmd_blocks(np.zeros((5, 3)), np.zeros((5, 2)), [([0, 2], [0, 2])])
    with pytest.raises(ValueError, match="block 1"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [[0], []])
    with pytest.raises(ValueError, match="block 0"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [([0, 1], [0])])
    with pytest.raises(ValueError, match="sigma"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [[0], [1]], sigma=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="scale"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [[0]], scale=[1.0])
    with pytest.raises(ValueError, match="circular"):
        ST.mmd_blocks(np.zeros((5, 2)), np.zeros((5, 2)), [[0]], circular=[True])


# ---- the solver -------------------------------------------------------------------------------------------------------------
def _fake_graph_solver(monkeypatch):
    """A solver whose graph is a pose prior and a range factor over {X0, L1}, eliminated but never trained: enough to reach
    the argument checks."""
    from slam.NFiSAM import NFiSAM
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    s.add_node(X0)
    s.add_node(L1)
    s.add_factor(F.UnarySE2ApproximateGaussianPriorFactor(X0, np.zeros(3), np.diag([1e-2, 1e-2, 1e-4])))
    s.add_factor(F.SE2R2RangeGaussianLikelihoodFactor(X0, L1, 3.0, 0.5))
    s.update_physical_and_working_graphs()
    refuse = Refuse()
    for name in ("mmd_sums", "mmd_sums_t", "_columns", "posterior_walk_raw", "upload"):
        monkeypatch.setattr(nh, name, refuse)
    return s, X0, L1, refuse


def test_posterior_mmd_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert ParallelNFiSAM.posterior_mmd is NFiSAM.posterior_mmd
    nh.build()
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().posterior_mmd({})
    s, X0, L1, refuse = _fake_graph_solver(monkeypatch)
    X9 = SE2Variable("X9")
    ref = {X0: np.zeros((9, 3)), L1: np.zeros((9, 2))}
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):      # a draw needs a trained tree
        s.posterior_mmd(ref)
    with pytest.raises(ValueError, match="estimator"):
        s.posterior_mmd(ref, own, estimator="MMD")
    with pytest.raises(ValueError, match="columns"):
        s.posterior_mmd(ref, own, columns="xyz")
    with pytest.raises(ValueError, match="no variable"):
        s.posterior_mmd({}, own)
    with pytest.raises(ValueError, match="reference lacks variable L1"):
        s.posterior_mmd({X0: ref[X0]}, own, variables=[X0, L1])
    with pytest.raises(ValueError, match="X9 is not in the elimination ordering"):
        s.posterior_mmd({**ref, X9: np.zeros((9, 3))}, own, variables=[X0, X9])
    with pytest.raises(ValueError, match="ragged reference"):
        s.posterior_mmd({X0: np.zeros((9, 3)), L1: np.zeros((8, 2))}, own)
    with pytest.raises(ValueError, match=r"reference samples of X0 must be \[m, 3\]"):
        s.posterior_mmd({X0: np.zeros((9, 2)), L1: np.zeros((9, 2))}, own)
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_mmd(ref, {X0: own[X0]})
    with pytest.raises(ValueError, match="ragged samples"):
        s.posterior_mmd(ref, {X0: np.zeros((7, 3)), L1: np.zeros((6, 2))})
    with pytest.raises(ValueError, match="samples of L1"):
        s.posterior_mmd(ref, {X0: np.zeros((7, 3)), L1: np.zeros((7, 3))})
    with pytest.raises(ValueError, match="block"):
        s.posterior_mmd(ref, own, variables=[X0], blocks=[(X0, L1)])
    with pytest.raises(ValueError, match="sigma"):
        s.posterior_mmd(ref, own, sigma=[1.0, 2.0])
    with pytest.raises(ValueError, match="at least 2 points"):
        s.posterior_mmd({X0: np.zeros((1, 3)), L1: np.zeros((1, 2))}, own)
    with pytest.raises(ValueError, match="at least 2 points"):
        s.posterior_mmd(ref, {X0: np.zeros((1, 3)), L1: np.zeros((1, 2))}, estimator="MMDu2")
    assert refuse.calls == 0
