"""The sliced Wasserstein distance without a GPU: the float64 numpy oracle (written out here, not taken from the project) and
what it rests on, the direction contract, the table packing, the struct against the header, and every refusal of the table
check, both binding forms, the statistics front, the solver and the C entry -- all before a device is needed.  The oracle,
the tolerance and the fixture of tests/test_sample_transport_gpu.py live here too."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from test_sample_mmd_cpu import Refuse, _fake_graph_solver
from utils import Statistics as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


# ---- shared with tests/test_sample_transport_gpu.py -----------------------------------------------------------------------------
def oracle_wpp(a, b, p):
    """W_p^p of the empirical measures of the SORTED keys a [m] and b [n]: the two quantile functions are steps that cut
    [0, 1] at i / m and j / n; on a piece between two neighbouring cuts both are constant.  In units of 1 / (m n)."""
    m, n = a.size, b.size
    cuts = np.union1d(np.arange(m + 1, dtype=np.int64) * n, np.arange(n + 1, dtype=np.int64) * m)
    left, width = cuts[:-1], np.diff(cuts)
    diff = np.abs(a[left // n] - b[left // m])
    return float(np.sum(width * (diff if p == 1 else diff * diff)) / (float(m) * float(n)))


def oracle_wpp_loops(a, b, p):
    """The same number by the double sum as the kernel is specified: j = floor(i n / m) .. ceil((i + 1) n / m) - 1,
    w_ij = min((i + 1) n, (j + 1) m) - max(i n, j m)."""
    m, n = a.size, b.size
    terms = []
    for i in range(m):
        for j in range(i * n // m, -((-(i + 1) * n) // m)):
            w = min((i + 1) * n, (j + 1) * m) - max(i * n, j * m)
            assert w > 0
            terms.append(w * abs(a[i] - b[j]) ** p)
    return math.fsum(terms) / (float(m) * float(n))


def oracle_keys(pts, cols, dirs, kind=None, scale=None):
    """The keys [n_dirs, points] of the float32 points along `dirs` [n_dirs, d], summed in ascending e in float64, and
    A1 = the largest sum_e |dir scale f(x)| over points and directions."""
    z = np.asarray(pts, dtype=np.float32).astype(np.float64)[:, np.asarray(cols)]
    if kind is not None:
        kind = np.asarray(kind)
        z = np.where(kind[None, :] == 1, np.cos(z), np.where(kind[None, :] == 2, np.sin(z), z))
    coef = np.asarray(dirs, dtype=np.float64) * (1.0 if scale is None else np.asarray(scale, dtype=np.float64)[None, :])
    keys, mag = np.zeros((coef.shape[0], z.shape[0])), np.zeros((coef.shape[0], z.shape[0]))
    for e in range(z.shape[1]):
        term = coef[:, e:e + 1] * z[None, :, e]
        keys += term
        mag += np.abs(term)
    return keys, float(mag.max())


def oracle_slices(x, y, xcols, ycols, dirs, p, kind=None, scale=None):
    """-> (slices [n_dirs] of W_p^p, A1 over both sets)."""
    kx, ax = oracle_keys(x, xcols, dirs, kind, scale)
    ky, ay = oracle_keys(y, ycols, dirs, kind, scale)
    return np.array([oracle_wpp(np.sort(a), np.sort(b), p) for a, b in zip(kx, ky)]), max(ax, ay)


def tolerance(ref, p, d, a1, m, n):
    """The issue's bound per slice, derived: a key carries at most (d + 1) eps A1 of rounding, a perturbation delta of the keys
    moves W_p^p by at most 2 p delta W_p^(p - 1) to first order, and the sum of m + n pieces adds (m + n) eps relative; the
    factor 4 is the margin for contraction and sort-order differences."""
    ref = np.asarray(ref, dtype=np.float64)
    return 4.0 * (2.0 * p * (d + 1) * EPS * a1 * ref ** ((p - 1.0) / p) + (m + n) * EPS * ref)


COLS = 44


def fixture(m, n, seed=31):
    """x [m, 44], y [n, 44] float32: coordinates near 100 with spreads of 1.5 and y shifted by 0.4 in columns 0..39, headings
    either side of the seam in columns 40 (x near +3.1, y near -3.1) and 41 (uniform), two more Gaussian columns, and -- where
    there is room -- duplicated rows (ties)."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((m, COLS)) * 1.5 + 100.0
    y = rng.standard_normal((n, COLS)) * 1.5 + 100.4
    x[:, 40] = ((rng.standard_normal(m) * 0.3 + 3.1) + np.pi) % (2 * np.pi) - np.pi
    y[:, 40] = ((rng.standard_normal(n) * 0.3 - 3.1) + np.pi) % (2 * np.pi) - np.pi
    x[:, 41] = rng.uniform(-np.pi, np.pi, m)
    y[:, 41] = rng.uniform(-np.pi, np.pi, n)
    if m > 8:
        x[5], x[m - 1] = x[3], x[3]
    if n > 8:
        y[7] = y[2]
    return x.astype(np.float32), y.astype(np.float32)


def table():
    """[(xcols, ycols, n_dirs, scale or None, kind or None)]: d in {1, 2, 7, 17, 40}, n_dirs in {1, 5, 64}, a block with a
    scale, one whose xcols differ from its ycols, and two with a heading either side of the seam (cos / sin entries)."""
    r = lambda a, b: list(range(a, b))                                                        # noqa: E731
    rng = np.random.RandomState(33)
    return [
        ([0], [0], 1, None, None), ([1, 2], [1, 2], 5, None, None), (r(3, 10), r(3, 10), 64, None, None),
        (r(10, 27), r(10, 27), 5, None, None), (r(0, 40), r(0, 40), 64, None, None),
        ([0, 1, 7], [0, 1, 7], 5, list(rng.uniform(0.5, 2.0, 3)), None),
        (r(9, 13), [12, 11, 10, 9], 5, None, None),
        ([3, 4, 40, 40], [3, 4, 40, 40], 64, None, [0, 0, 1, 2]),
        ([40, 40], [40, 40], 5, None, [1, 2]), ([41, 41, 42], [41, 41, 43], 5, [1.0, 1.0, 0.25], [1, 2, 0]),
    ]


def directions(tab, seed=0):
    return [ST.transport_directions(len(b[0]), b[2], seed) for b in tab]


def arrays(tab, dirs=None):
    """-> (blocks, xcols, ycols, dirs flat, kind or None, scale or None) of the table `tab`."""
    dirs = directions(tab) if dirs is None else dirs
    blocks = nh.pack_transport_blocks([len(b[0]) for b in tab], [d.shape[0] for d in dirs])
    xcols = np.concatenate([b[0] for b in tab]).astype(np.int32)
    ycols = np.concatenate([b[1] for b in tab]).astype(np.int32)
    scale = np.concatenate([np.ones(len(b[0])) if b[3] is None else np.asarray(b[3], dtype=np.float64) for b in tab]) \
        if any(b[3] is not None for b in tab) else None
    kind = np.concatenate([np.zeros(len(b[0]), dtype=np.uint8) if b[4] is None else np.asarray(b[4], dtype=np.uint8)
                           for b in tab]) if any(b[4] is not None for b in tab) else None
    return blocks, xcols, ycols, np.concatenate([d.reshape(-1) for d in dirs]), kind, scale


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(130, 200), (257, 255)])
@pytest.mark.parametrize("p", [1, 2])
def test_oracle_equals_the_equal_size_formula_on_replicated_sets(m, n, p):
    """Both sets replicated to lcm(m, n) points have the same quantile functions; there the distance is the mean of the
    differences of the order statistics.  The double sum of the specification is the same number."""
    rng = np.random.RandomState(m + p)
    a, b = np.sort(rng.standard_normal(m) * 1.5 + 100.0), np.sort(rng.standard_normal(n) * 1.5 + 100.4)
    L = m * n // math.gcd(m, n)
    ra, rb = np.repeat(a, L // m), np.repeat(b, L // n)
    want = math.fsum((np.abs(ra - rb) ** p).tolist()) / L
    got = oracle_wpp(a, b, p)
    assert abs(got - want) <= 64 * EPS * want, (got, want)
    assert abs(oracle_wpp_loops(a, b, p) - want) <= 64 * EPS * want
    assert oracle_wpp(a, b, p) == oracle_wpp(b, a, p)


@pytest.mark.parametrize("m,n", [(1, 1), (1, 3), (64, 64), (65, 64), (130, 200), (257, 255)])
def test_oracle_equals_scipy_for_p_1(m, n):
    from scipy.stats import wasserstein_distance
    rng = np.random.RandomState(7 * m + n)
    a, b = rng.standard_normal(m) * 1.5 + 100.0, rng.standard_normal(n) * 1.5 + 100.4
    a[: m // 3] = a[0]                                                              # ties
    want = wasserstein_distance(a, b)
    assert abs(oracle_wpp(np.sort(a), np.sort(b), 1) - want) <= 64 * EPS * max(want, 1.0)


@pytest.mark.parametrize("p", [1, 2])
def test_oracle_reduces_to_the_order_statistics_for_equal_sizes(p):
    rng = np.random.RandomState(3)
    a, b = np.sort(rng.standard_normal(97)), np.sort(rng.standard_normal(97) + 0.5)
    want = math.fsum((np.abs(a - b) ** p).tolist()) / 97
    assert abs(oracle_wpp(a, b, p) - want) <= 8 * EPS * want
    assert oracle_wpp(a, a.copy(), p) == 0.0 and oracle_wpp(a, np.repeat(a, 2), p) == 0.0


def test_oracle_keys_and_the_chord_embedding():
    """A heading either side of the seam: the cos / sin entries put 3.1 and -3.1 at a chord of 2 sin(0.0416), not 6.2 apart."""
    x = np.array([[3.1]], dtype=np.float32)
    y = np.array([[-3.1]], dtype=np.float32)
    dirs = np.eye(2)
    s, a1 = oracle_slices(x, y, [0, 0], [0, 0], dirs, 2, kind=[1, 2])
    gap = 2 * np.pi - 2 * float(np.float32(3.1))
    assert abs(math.sqrt(s.sum()) - 2.0 * math.sin(gap / 2.0)) <= 1e-15 and a1 <= 1.0
    assert abs(math.sqrt(s.sum()) - gap) <= gap ** 3 / 24.0 + 1e-15                  # the radian difference, to third order


# ---- the directions and the algebra -------------------------------------------------------------------------------------------
def test_transport_directions_contract():
    for d in (2, 7, 40):
        D = ST.transport_directions(d, 64, seed=0)
        assert D.shape == (64, d) and D.dtype == np.float64
        np.testing.assert_allclose((D * D).sum(1), 1.0, rtol=0, atol=4 * EPS)
        assert np.array_equal(D, ST.transport_directions(d, 64, seed=0))
        assert not np.array_equal(D, ST.transport_directions(d, 64, seed=1))
        g = np.random.default_rng([0, d]).standard_normal((64, d))
        assert np.array_equal(D, g / np.sqrt((g * g).sum(1))[:, None])
    assert not np.array_equal(ST.transport_directions(3, 4, 0)[:, :2], ST.transport_directions(2, 4, 0))
    for count in (1, 5, 64):
        assert np.array_equal(ST.transport_directions(1, count, seed=9), [[1.0]])
    for bad in ((0, 4, 0), (2, 0, 0), (2, 4, -1)):
        with pytest.raises(ValueError, match="transport_directions"):
            ST.transport_directions(*bad)
    # a block's directions do not depend on its place in a table
    tab = ST.transport_tables([(np.arange(3), np.arange(3), np.zeros(3, np.uint8)), (np.arange(2), np.arange(2), np.zeros(2, np.uint8)),
                               (np.arange(3) + 4, np.arange(3), np.zeros(3, np.uint8))], 6, 5, False)
    assert np.array_equal(tab["dirs"][:18], tab["dirs"][30:48]) and np.array_equal(tab["dirs"][:18].reshape(6, 3),
                                                                                  ST.transport_directions(3, 6, 5))


def test_wasserstein_from_slices():
    assert ST.wasserstein_from_slices([4.0, 9.0, 2.0], 2) == (math.sqrt(5.0), 3.0)
    assert ST.wasserstein_from_slices([4.0, 9.0, 2.0], 1) == (5.0, 9.0)
    assert ST.wasserstein_from_slices([0.0], 2) == (0.0, 0.0)
    assert all(np.isnan(v) for v in ST.wasserstein_from_slices([1.0, np.nan], 2))
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        ST.wasserstein_from_slices([1.0], 3)
    with pytest.raises(ValueError, match="no slices"):
        ST.wasserstein_from_slices([], 2)


def test_pack_transport_blocks_offsets():
    t = nh.pack_transport_blocks([3, 1, 40], [5, 1, 64])
    assert t.dtype == nh.TRANSPORT_BLOCK_DTYPE
    assert t["col_off"].tolist() == [0, 3, 4] and t["d"].tolist() == [3, 1, 40] and t["n_dirs"].tolist() == [5, 1, 64]
    assert t["dir_off"].tolist() == [0, 15, 16] and t["out_off"].tolist() == [0, 5, 6] and t["reserved"].tolist() == [0, 0, 0]
    assert nh.pack_transport_blocks([2, 2], 7)["dir_off"].tolist() == [0, 14]
    with pytest.raises(ValueError, match="n_dirs"):
        nh.pack_transport_blocks([2, 2], [7, 7, 7])


def test_transport_tables_axes_and_entries():
    ent = ST.transport_entries([(np.array([0, 2]), np.array([1, 3])), (np.array([2]), np.array([3]))], np.array([False, False, True]))
    assert [e[0].tolist() for e in ent] == [[0, 2, 2], [2, 2]] and [e[1].tolist() for e in ent] == [[1, 3, 3], [3, 3]]
    assert [e[2].tolist() for e in ent] == [[0, 1, 2], [1, 2]]
    tab = ST.transport_tables(ent, 4, 0, [False, True], scale=[2.0, 1.0, 0.5])
    t = tab["blocks"]
    assert tab["main"] == 2 and tab["axis_at"] == {1: 2} and t["d"].tolist() == [3, 2, 1, 1] and t["n_dirs"].tolist() == [4, 4, 1, 1]
    assert t["col_off"].tolist() == [0, 3, 3, 4] and t["out_off"].tolist() == [0, 4, 8, 9] and t["dir_off"].tolist() == [0, 12, 20, 21]
    assert tab["dirs"].size == 22 and tab["dirs"][20:].tolist() == [1.0, 1.0] and tab["scale"].tolist() == [2.0, 0.5, 0.5, 0.5, 0.5]
    assert tab["kind"].tolist() == [0, 1, 2, 1, 2]
    nh.check_transport_blocks(t, tab["xcols"], tab["ycols"], 3, 4, tab["dirs"], tab["kind"], tab["scale"])
    res = ST.transport_result(np.array([1.0, 4.0, 9.0, 2.0, 0.0, 0.0, 0.0, 16.0, 25.0, 36.0]), tab, 2)
    assert res["distance"].tolist() == [2.0, 2.0] and res["max_sliced"].tolist() == [3.0, 4.0]
    assert res["axis"][0] is None and res["axis"][1].tolist() == [5.0, 6.0] and res["slices"][1].tolist() == [0.0, 0.0, 0.0, 16.0]
    with pytest.raises(ValueError, match="65535"):
        ST.transport_tables([(np.arange(40000), np.arange(40000), np.zeros(40000, np.uint8))] * 2, 1, 0, True)


def test_struct_size_is_32_and_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    names = ("col_off", "d", "n_dirs", "reserved", "dir_off", "out_off")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nfisam_hip.h"\nint main(void) { '
                   'printf("%zu ' + "%zu " * len(names) + '%d\\n", sizeof(nfisam_transport_block), '
                   + ", ".join("offsetof(nfisam_transport_block, %s)" % k for k in names) + ', NFISAM_TRANSPORT_MAX_N); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [32, 0, 4, 8, 12, 16, 24, 8192]
    assert sizes[:-1] == [C.sizeof(nh.TransportBlock)] + [getattr(nh.TransportBlock, k).offset for k in names]
    assert nh.TRANSPORT_BLOCK_DTYPE.itemsize == 32 and nh.TRANSPORT_MAX_N == 8192
    assert [nh.TRANSPORT_BLOCK_DTYPE.fields[k][1] for k in names] == sizes[1:-1]


# ---- refusals before a device is needed -----------------------------------------------------------------------------------------
def test_check_transport_blocks_refusals():
    t = nh.pack_transport_blocks([2, 1], [3, 1])
    dirs = np.concatenate([ST.transport_directions(2, 3, 0).reshape(-1), [1.0]])
    assert nh.check_transport_blocks(t, [0, 1, 2], [2, 1, 0], 3, 3, dirs, [0, 1, 2], [1.0, 2.0, 3.0]) == 4

    def refuse(match, blocks=t, xcols=(0, 1, 2), ycols=(2, 1, 0), x_rows=3, y_rows=3, d=dirs, kind=None, scale=None):
        with pytest.raises(ValueError, match=match):
            nh.check_transport_blocks(blocks, list(xcols), list(ycols), x_rows, y_rows, d, kind, scale)

    refuse("TRANSPORT_BLOCK_DTYPE", blocks=nh.pack_mmd_blocks([2, 1], [1.0, 1.0]))
    refuse("1..65535 blocks", blocks=t[:0])
    refuse("same length", ycols=(0, 1))
    refuse("xcols: a row is out of range", x_rows=2)
    refuse("ycols: a row is out of range", ycols=(0, 1, -1))
    refuse("kind must have one value per entry", kind=[0, 1])
    refuse("scale must have one value per entry", scale=[1.0])
    refuse("kind must be 0", kind=[0, 1, 3])
    refuse("scale must be finite", scale=[1.0, np.inf, 1.0])
    refuse("dirs must be finite", d=np.where(np.arange(7) == 2, np.nan, dirs))
    refuse("dirs has 6 values, the table names 7", d=dirs[:6])
    refuse("dirs has 8 values, the table names 7", d=np.concatenate([dirs, [1.0]]))
    refuse("1-D float array", d=dirs.reshape(1, -1))
    refuse("1-D float array", d=np.arange(7))
    for field, value, match in (("d", 0, "entries"), ("col_off", 3, "entries"), ("col_off", -1, "entries"), ("n_dirs", 0, "n_dirs = 0"),
                                ("n_dirs", 65536, "n_dirs = 65536"), ("dir_off", -1, "dirs has"), ("dir_off", 2, "dirs has"),
                                ("out_off", -1, "out_off"), ("out_off", 2, "share an entry")):
        bad = t.copy()
        bad[field][0 if field != "col_off" else 1] = value
        refuse(match, blocks=bad)


def test_the_binding_refuses_before_any_copy(monkeypatch):
    refuse = Refuse()
    for name in ("upload", "_columns"):
        monkeypatch.setattr(nh, name, refuse)
    t = nh.pack_transport_blocks([2], [3])
    dirs = ST.transport_directions(2, 3, 0).reshape(-1)
    X, Y = np.zeros((5, 3), dtype=np.float32), np.zeros((6, 3), dtype=np.float32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sliced_transport(torch.zeros(5, 3), torch.zeros(6, 3), t, [0, 1], [0, 1], dirs)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sliced_transport(X, Y, t, [0, 1], [0, 1], dirs, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        nh.sliced_transport_t(torch.zeros(3, 5), torch.zeros(3, 6), t, [0, 1], [0, 1], dirs)
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        nh.sliced_transport(X[0], Y, t, [0, 1], [0, 1], dirs, device="cuda")
    with pytest.raises(ValueError, match="xcols"):
        nh.sliced_transport(X, Y, t, [0, 3], [0, 1], dirs, device="cuda")
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        nh.sliced_transport(X, Y, t, [0, 1], [0, 1], dirs, p=3, device="cuda")
    with pytest.raises(ValueError, match="at least one point"):
        nh.sliced_transport(X[:0], Y, t, [0, 1], [0, 1], dirs, device="cuda")
    with pytest.raises(ValueError, match="at most 8192 points"):
        nh.sliced_transport(np.zeros((8193, 3), dtype=np.float32), Y, t, [0, 1], [0, 1], dirs, device="cuda")
    with pytest.raises(ValueError, match="at most 8192 points"):
        nh.sliced_transport(X, np.zeros((8193, 3), dtype=np.float32), t, [0, 1], [0, 1], dirs, device="cuda")
    with pytest.raises(ValueError, match="kind must be 0"):
        nh.sliced_transport(X, Y, t, [0, 1], [0, 1], dirs, kind=[0, 9], device="cuda")
    with pytest.raises(ValueError, match="dirs has"):
        nh.sliced_transport(X, Y, t, [0, 1], [0, 1], dirs[:4], device="cuda")
    with pytest.raises(ValueError, match="dirs must be finite"):
        nh.sliced_transport(X, Y, t, [0, 1], [0, 1], dirs * np.inf, device="cuda")
    with pytest.raises(ValueError, match="scale must be finite"):
        nh.sliced_transport(X, Y, t, [0, 1], [0, 1], dirs, scale=[1.0, np.nan], device="cuda")
    assert refuse.calls == 0


def test_sliced_wasserstein_refuses_before_any_copy(monkeypatch):
    refuse = Refuse()
    for name in ("upload", "_columns", "sliced_transport", "sliced_transport_t"):
        monkeypatch.setattr(nh, name, refuse)
    x, y = np.zeros((5, 3), dtype=np.float32), np.zeros((6, 3), dtype=np.float32)
    for kwargs, match in ((dict(p=3), "p must be 1 or 2"), (dict(p=0), "p must be 1 or 2"), (dict(directions=0), "directions"),
                          (dict(directions=65536), "directions"), (dict(directions=2.5), "directions"), (dict(seed=-1), "seed"),
                          (dict(seed=0.5), "seed"), (dict(scale=np.ones(2)), "scale"), (dict(scale=[1.0, np.nan, 1.0]), "scale"),
                          (dict(circular=[True]), "circular"), (dict(axes=[True, False]), "axes")):
        with pytest.raises(ValueError, match=match):
            ST.sliced_wasserstein(x, y, [[0, 1]], **kwargs)
        with pytest.raises(ValueError, match=match):
            ST.sliced_wasserstein_t(torch.zeros(3, 5), torch.zeros(3, 6), [[0, 1]], **kwargs)
    with pytest.raises(ValueError, match="outside"):
        ST.sliced_wasserstein(x, y, [[0, 3]])
    with pytest.raises(ValueError, match="outside"):
        ST.sliced_wasserstein(x, y, [([0, 1], [0, 3])])
    with pytest.raises(ValueError, match="no blocks"):
        ST.sliced_wasserstein(x, y, [])
    with pytest.raises(ValueError, match="block 0"):
        ST.sliced_wasserstein(x, y, [[]])
    with pytest.raises(ValueError, match=r"\[points, columns\]"):
        ST.sliced_wasserstein(x[0], y, [[0]])
    with pytest.raises(ValueError, match=r"\[columns, points\]"):
        ST.sliced_wasserstein_t(torch.zeros(3), torch.zeros(3, 6), [[0]])
    with pytest.raises(ValueError, match="m = 0 points"):
        ST.sliced_wasserstein(x[:0], y, [[0]])
    with pytest.raises(ValueError, match="n = 8193 points"):
        ST.sliced_wasserstein(x, np.zeros((8193, 3), dtype=np.float32), [[0]])
    assert refuse.calls == 0


def test_posterior_transport_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    from slam.Variables import SE2Variable
    assert ParallelNFiSAM.posterior_transport is NFiSAM.posterior_transport
    nh.build()
    with pytest.raises(RuntimeError, match="no factor graph"):
        NFiSAM().posterior_transport({})
    s, X0, L1, refuse = _fake_graph_solver(monkeypatch)
    for name in ("sliced_transport", "sliced_transport_t"):
        monkeypatch.setattr(nh, name, refuse)
    ref = {X0: np.zeros((9, 3)), L1: np.zeros((9, 2))}
    own = {X0: np.zeros((7, 3)), L1: np.zeros((7, 2))}
    with pytest.raises(RuntimeError, match="no Bayes tree|no trained model"):      # a draw needs a trained tree
        s.posterior_transport(ref)
    # the option checks fire before the front: with nothing to draw from, they still come first
    for kwargs, match in ((dict(p=3), "p must be 1 or 2"), (dict(directions=0), "directions"), (dict(seed=-2), "seed"),
                          (dict(columns="z"), "columns")):
        with pytest.raises(ValueError, match="posterior_transport: .*" + match):
            s.posterior_transport(ref, **kwargs)
        with pytest.raises(ValueError, match="posterior_transport: .*" + match):
            s.posterior_transport(ref, own, **kwargs)
    for kwargs, match in ((dict(variables=[]), "no variable"), (dict(blocks=[()]), "block"), (dict(blocks=[(X0, X0)], variables=[L1]), "block"),
                          (dict(variables=[SE2Variable("X9")]), "not in the elimination ordering")):
        with pytest.raises(ValueError, match="posterior_transport: .*" + match):
            s.posterior_transport(ref, own, **kwargs)
    with pytest.raises(ValueError, match="reference lacks variable L1"):
        s.posterior_transport({X0: ref[X0]}, own, variables=[X0, L1])
    with pytest.raises(ValueError, match="samples lack variable L1"):
        s.posterior_transport(ref, {X0: own[X0]})
    with pytest.raises(ValueError, match=r"reference samples of X0 must be \[m, 3\]"):
        s.posterior_transport({X0: np.zeros((9, 2)), L1: ref[L1]}, own)
    with pytest.raises(ValueError, match="ragged reference"):
        s.posterior_transport({X0: ref[X0], L1: ref[L1][:8]}, own)
    with pytest.raises(ValueError, match="the reference set has 0 points"):
        s.posterior_transport({X0: ref[X0][:0], L1: ref[L1][:0]}, own)
    with pytest.raises(ValueError, match="the reference set has 8193 points"):
        s.posterior_transport({X0: np.zeros((8193, 3)), L1: np.zeros((8193, 2))}, own)
    with pytest.raises(ValueError, match="the posterior set has 8193 points"):
        s.posterior_transport(ref, {X0: np.zeros((8193, 3)), L1: np.zeros((8193, 2))})
    assert refuse.calls == 0


def test_library_exports_the_entry_and_the_c_entry_refuses_on_the_host():
    """Every NFISAM_ERR_ARG case, on the host, before the device is touched (the pointers below are never dereferenced: they
    are not device memory)."""
    nh.build()
    lib = nh.lib()
    assert "nfisam_sample_sliced_transport" in nh.EXPORTS and hasattr(lib, "nfisam_sample_sliced_transport")
    assert lib.nfisam_abi_version() == 1600
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    assert "int nfisam_sample_sliced_transport(" in hdr and "#define NFISAM_TRANSPORT_MAX_N %d" % nh.TRANSPORT_MAX_N in hdr
    assert "sample_transport" in open(os.path.join(ROOT, "nf-isam_amd", "csrc", "Makefile")).read()
    blocks = nh.pack_transport_blocks([2, 1], [3, 1])
    fake = C.c_void_p(4096)

    def call(Xt=fake, x_rows=4, m=5, Yt=fake, y_rows=4, n=5, blk=blocks, blk_dev=fake, nb=2, xcols=fake, ycols=fake, kind=None,
             scale=None, ne=3, dirs=fake, dirs_count=7, p=2, out=fake, out_count=4):
        return lib.nfisam_sample_sliced_transport(Xt, x_rows, m, Yt, y_rows, n, None if blk is None else blk.ctypes.data_as(C.c_void_p),
                                                  blk_dev, nb, xcols, ycols, kind, scale, ne, dirs, dirs_count, p, out, out_count,
                                                  None)
    for name in ("Xt", "Yt", "blk", "blk_dev", "xcols", "ycols", "dirs", "out"):
        assert call(**{name: None}) == nh.ERR_ARG, name
    for name in ("m", "n", "x_rows", "y_rows", "ne", "nb"):
        assert call(**{name: 0}) == nh.ERR_ARG and call(**{name: -1}) == nh.ERR_ARG, name
    assert call(m=8193) == nh.ERR_ARG and call(n=8193) == nh.ERR_ARG
    assert call(p=0) == nh.ERR_ARG and call(p=3) == nh.ERR_ARG
    assert call(nb=65536) == nh.ERR_ARG
    assert call(dirs_count=6) == nh.ERR_ARG and call(out_count=3) == nh.ERR_ARG and call(dirs_count=0) == nh.ERR_ARG
    for field, value in (("d", 0), ("d", -1), ("n_dirs", 0), ("n_dirs", 65536), ("dir_off", -1), ("dir_off", 2), ("out_off", -1),
                         ("out_off", 2), ("dir_off", 2 ** 62), ("out_off", 2 ** 62)):
        bad = blocks.copy()
        bad[field][0] = value
        assert call(blk=bad) == nh.ERR_ARG, (field, value)
