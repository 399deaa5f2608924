"""The device's Hessian-vector products (nfisam_factor_graph_hvp) against the 60-digit Hessians of
tests/golden/factor_hessian_exact.npz, with the bound and the constant of tests/test_factor_exact_cpu.py and no allowance:

    |device - exact| <= C x 2^-53 x scale,   C = 256

then what is built on the entry: the matrix-free solvers of utils/Statistics.py on a quadratic graph, and the solver's
`joint_hessian_product`, `map_newton` and `laplace_approximation` on the small range problem.  The tables are built like those
of tests/test_factor_exact_gpu.py; column c of a factor's block is the product along e_c over that factor's own columns.  The
largest ratio per case is printed; the MI355X's are in profiles/factor_hessian.json next to the host's (largest: 6.4 over the
cases, on se2_prior_medium, and 2.1 on the joint H v of Manhattan-136)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from test_factor_density_gpu import _case_table
from test_factor_exact_cpu import C, EPS, GOLDEN, ratio
from test_factor_hessian_cpu import hessian_cases, hessian_fixture, hessian_graph
from utils import Statistics as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_SINGLE = 80


def _columns(f, r):
    return np.concatenate([np.arange(r[v], r[v] + v.dim) for v in f.vars])


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


# ---- 1. every case with one factor -----------------------------------------------------------------------------------------------------
def test_single_factor_cases_every_column_of_every_block():
    cases = [c for c in hessian_cases() if len(c.factors) == 1]
    assert len(cases) >= 28 + 15
    terms, rows, total = _case_table([(c.cls, c.factors[0], c.x, None) for c in cases])
    assert set(terms["code"]) == set(nh.FAC_CODES.values())                      # every device code is exercised
    n, widest = N_SINGLE, max(c.x.shape[1] for c in cases)
    gather = nh.pack_score_gather(terms, total)
    S = np.zeros((n, total), dtype=np.float32)
    for c, r in zip(cases, rows):
        S[:, _columns(c.factors[0], r)] = c.x[np.arange(n) % c.x.shape[0]]
    blocks = [np.zeros((n, c.x.shape[1], c.x.shape[1])) for c in cases]
    for k in range(widest):                                                      # one launch per column, n = 80 < 1024
        V = np.zeros((n, total))
        for c, r in zip(cases, rows):
            if k < c.x.shape[1]:
                V[:, _columns(c.factors[0], r)[k]] = 1.0
        H = nh.factor_graph_hvp(terms, S, V, DEV, gather=gather)
        assert H.dtype == torch.float64 and tuple(H.shape) == (n, total)
        H = H.cpu().numpy()
        for b, c, r in zip(blocks, cases, rows):
            if k < c.x.shape[1]:
                b[:, :, k] = H[:, _columns(c.factors[0], r)]
    worst = {}
    for b, c in zip(blocks, cases):
        idx = np.arange(n) % c.x.shape[0]
        m = c.mask[idx]
        assert np.all(np.isfinite(b)), c.name                                    # finite everywhere, masked rows included
        worst[c.name] = ratio(b[m], c.hess[idx][m], c.hess_scale[idx][m])
        assert ratio(b[m].transpose(0, 2, 1), b[m], 2.0 * c.hess_scale[idx][m]) <= C, c.name     # symmetric within the bound
        if not isinstance(c.factors[0], F.BinaryFactorMixture):
            assert not b[~m].any(), c.name                                       # a range of exactly 0: the zero vector
        print("%-26s %-42s |device - exact| / (2^-53 scale): %8.3g" % (c.name, c.cls, worst[c.name]))
    print("largest over %d cases: %.3g (C = %g)" % (len(cases), max(worst.values()), C))
    bad = {k: v for k, v in worst.items() if v > C}
    assert not bad, bad


# ---- 2. the score output, bit stability ------------------------------------------------------------------------------------------------
def _ksd_table():
    factors, col, x, v, hv, scale = hessian_graph(hessian_fixture(), "ksd")
    terms = nh.pack_factor_terms(factors, col)
    return terms, nh.pack_score_gather(terms, x.shape[1]), x, v, hv, scale


def test_score_output_is_the_score_entry_bit_for_bit():
    terms, gather, x, v, _, _ = _ksd_table()
    n = 130
    rng = np.random.RandomState(5)
    St = _t(x[np.arange(n) % x.shape[0]].T, np.float32)
    Vt = _t(rng.randn(x.shape[1], n), np.float64)
    Gt = nh.factor_graph_score_t(terms, St, DEV, gather=gather)
    Ht = nh.factor_graph_hvp_t(terms, St, Vt, DEV, gather=gather)
    Ht2, Gt2, slots = nh.factor_graph_hvp_t(terms, St, Vt, DEV, gather=gather, score=True, slots=True)
    assert torch.equal(Gt2, Gt) and torch.equal(Ht2, Ht)                         # same bits, with and without the score
    assert tuple(slots.shape) == (gather["n_slots"], n) and torch.all(torch.isfinite(Ht)) and Ht.abs().max() > 0
    again = nh.factor_graph_hvp_t(terms, St, Vt, DEV, gather=gather, score=True)
    assert torch.equal(again[0], Ht) and torch.equal(again[1], Gt)               # a second call: the same bits
    # the mixture's two candidates and the twice-listed candidate of `mix_twice` add through the gather: rows with two slots
    assert max(np.diff(gather["row_off"])) >= 2
    # row-major front: the same numbers
    H = nh.factor_graph_hvp(terms, St.t(), Vt.t(), DEV, gather=gather)
    assert torch.equal(H, Ht.t())
    # a point's column alone and among others
    for m in (1, 64, 65, 130):
        part = nh.factor_graph_hvp_t(terms, St[:, :m].contiguous(), Vt[:, :m].contiguous(), DEV, gather=gather)
        assert torch.equal(part, Ht[:, :m]), m
    last = nh.factor_graph_hvp_t(terms, St[:, 129:].contiguous(), Vt[:, 129:].contiguous(), DEV, gather=gather)
    assert torch.equal(last, Ht[:, 129:])


def test_binding_refusals_before_any_launch():
    terms, gather, x, _, _, _ = _ksd_table()
    St = _t(x[:8].T, np.float32)
    Vt = torch.zeros(13, 8, dtype=torch.float64, device=DEV)
    for bad in (Vt.float(), Vt[:, :7].contiguous(), Vt.t().contiguous().t(), Vt.cpu(), Vt.cpu().numpy(), None):
        with pytest.raises(ValueError):
            nh.factor_graph_hvp_t(terms, St, bad, DEV, gather=gather)
    with pytest.raises(ValueError):
        nh.factor_graph_hvp_t(terms, St.double(), Vt, DEV, gather=gather)
    with pytest.raises(ValueError):
        nh.factor_graph_hvp_t(terms[:3], St, Vt, DEV, gather=gather)             # gather packed for another table
    with pytest.raises(ValueError):
        nh.factor_graph_hvp(terms, x[:8], np.zeros((8, 12)), DEV)
    bad_terms = terms.copy()
    bad_terms["a"][0] = 12
    with pytest.raises(ValueError):
        nh.factor_graph_hvp_t(bad_terms, St, Vt, DEV)                            # the table's own check


# ---- 3. the SE(2) sweeps: one observation per point ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["se2_prior", "se2_rel"])
def test_se2_sweeps_one_observation_per_point(kind):
    """As in tests/test_factor_exact_gpu.py: all factors of a kind share the rows of one pose (two poses), factor i is graded at
    point i through its own slots.  Rows with |w| >= 1e-3 and rows below the series switch of a'' and l'' (|w| < 0.6) are both
    graded with no allowance."""
    cases = [c for c in hessian_cases() if c.name.startswith(kind)]
    assert [c.name for c in cases][:3] == [kind + "_" + t for t in ("tight", "medium", "full")]
    width = cases[0].x.shape[1]
    factors = [f for c in cases for f in c.factors]
    terms = np.concatenate([nh.pack_factor_terms([f], {v: 3 * j for j, v in enumerate(f.vars)}) for f in factors])
    gather = nh.pack_score_gather(terms, width)
    S = np.concatenate([c.x for c in cases])
    n = S.shape[0]
    assert n == len(factors) and 64 < n <= 192
    blocks = np.zeros((n, width, width))
    for k in range(width):
        V = np.zeros((n, width))
        V[:, k] = 1.0
        slots = nh.factor_graph_hvp(terms, S, V, DEV, gather=gather, slots=True)[1].cpu().numpy()
        blocks[:, :, k] = np.stack([slots[gather["slot_off"][i]:gather["slot_off"][i] + width, i] for i in range(n)])
    assert np.all(np.isfinite(blocks))
    off, bad, counts = 0, {}, np.zeros(2, dtype=int)
    for c in cases:
        m = c.x.shape[0]
        b = blocks[off:off + m]
        r = ratio(b, c.hess, c.hess_scale)
        print("%-26s %-42s |device - exact| / (2^-53 scale): %8.3g" % (c.name, c.cls, r))
        if r > C:
            bad[c.name] = r
        big, series = np.abs(c.w) >= 1e-3, np.abs(c.w) < 2.0 * F._SERIES2_H
        assert ratio(b[big], c.hess[big], c.hess_scale[big]) <= C and ratio(b[series], c.hess[series], c.hess_scale[series]) <= C
        counts += (int(big.sum()), int(series.sum()))
        off += m
    assert not bad, bad
    assert counts[0] >= 45 and counts[1] >= 45


# ---- 4. whole graphs through the packers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["ksd", "manhattan136"])
def test_whole_graphs_through_the_packers(key):
    factors, col, x, v, hv, scale = hessian_graph(hessian_fixture(), key)
    terms = nh.pack_factor_terms(factors, col)
    gather = nh.pack_score_gather(terms, x.shape[1])
    H, G = nh.factor_graph_hvp(terms, x, np.broadcast_to(v, x.shape), DEV, gather=gather, score=True)
    assert torch.equal(G, nh.factor_graph_score(terms, x, DEV, gather=gather))
    r = ratio(H.cpu().numpy(), hv, scale)
    print("%s: %d factors x %d points: |device H v - exact| / (2^-53 scale): %.3g" % (key, len(factors), x.shape[0], r))
    assert r <= C


def test_twice_listed_candidate_adds_through_the_gather():
    c, = hessian_cases(names={"mix_twice"})
    f = c.factors[0]
    r = {}
    for v in f.vars:
        r[v] = sum(u.dim for u in r)
    terms = nh.pack_factor_terms([f], r)
    gather = nh.pack_score_gather(terms, c.x.shape[1])
    assert gather["n_slots"] == 8 and max(np.diff(gather["row_off"])) == 2       # L0's rows: two slots each
    rng = np.random.RandomState(9)
    V = rng.randn(*c.x.shape)
    H = nh.factor_graph_hvp(terms, c.x, V, DEV, gather=gather).cpu().numpy()
    exact = np.einsum("nrc,nc->nr", c.hess, V)
    bound = np.einsum("nrc,nc->nr", c.hess_scale, np.abs(V))                      # the product: the sum of its summands' bounds
    assert ratio(H, exact, bound) <= C


# ---- 5. the guard, the refusals of the C entry, empty inputs ---------------------------------------------------------------------------------
def test_one_guard_serves_the_hessian_entry_too():
    """The construction of tests/test_factor_score_gpu.py::test_one_guard_serves_both_entries: ten records in two FAC_RUN runs,
    eight of them bad, straight into the C entry.  St AND Vt are the middles of larger tensors whose outer rows hold a sentinel
    no result may show; a bad record owns NaN in its slots (of H v and of the score) and reads nothing; the good records keep
    the bits of the table without the bad ones.  Every index stays inside the allocations."""
    X, L0, L1 = SE2Variable("X0"), R2Variable("L0", VariableType.Landmark), R2Variable("L1", VariableType.Landmark)
    good = nh.pack_factor_terms([F.SE2R2RangeGaussianLikelihoodFactor(X, L0, 4.0, 0.5),
                                 F.UnaryR2GaussianPriorFactor(L1, np.array([1.0, -2.0]), np.diag([0.04, 0.09]))],
                                {X: 0, L0: 3, L1: 5})
    total, n, sentinel = 7, 65, 1.0e30

    def rec(code, a=0, b=0, k=0, cand=(0, 0, 0, 0)):
        t = np.zeros(1, dtype=nh.FACTOR_DTYPE)
        t["code"], t["a"], t["b"], t["k"], t["cand"] = code if isinstance(code, int) else nh.FAC_CODES[code], a, b, k, cand
        t["p"][0, :10] = [1.0, 0.5, 0.1, 2.0, 0.1, 0.2, 3.0, 0.3, 4.0, -1.0]
        return t
    bad = [rec("RANGE", a=-1, b=3), rec("PRIOR_SE2", a=5), rec("REL_SE2", a=0, b=5), rec("RANGE", a=0, b=6),
           rec("RANGE_MIX", k=0, cand=(3, 3, 3, 3)), rec("RANGE_MIX", k=5, cand=(3, 3, 3, 3)),
           rec("RANGE_MIX", k=2, cand=(3, 6, 0, 0)), rec(8)]
    owned = [4, 3, 6, 4, 0, 0, 6, 0]                                          # slot_count of the code and k
    for t in bad:
        with pytest.raises(ValueError):
            nh.check_factor_terms(t, total)
    terms = np.concatenate([good[:1]] + bad + [good[1:]])
    rng = np.random.RandomState(3)
    big = torch.full((11, n), sentinel, dtype=torch.float32, device=DEV)
    big[2:9] = _t(rng.randn(total, n) * 2.0, np.float32)
    bigv = torch.full((11, n), sentinel, dtype=torch.float64, device=DEV)
    bigv[2:9] = _t(rng.randn(total, n), np.float64)
    St, Vt = big[2:9], bigv[2:9]
    assert St.is_contiguous() and Vt.is_contiguous()
    ptr, null = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(0)

    def hvp(tb, stride, score):
        nt, ns = tb.shape[0], stride * tb.shape[0]
        dev = nh._upload_named(DEV, terms=nh._table_bytes(tb), slot_off=stride * np.arange(nt, dtype=np.int32),
                               row_off=np.zeros(total + 1, dtype=np.int32), row_slot=np.zeros(1, dtype=np.int32))
        Ht = torch.full((total, n), sentinel, dtype=torch.float64, device=DEV)
        Gt = torch.full((total, n), sentinel, dtype=torch.float64, device=DEV)
        count = int(nh.lib().nfisam_factor_graph_hvp_scratch_count(ns, n, int(score)))
        assert count == ns * n * (2 if score else 1)
        scratch = torch.full((count // n, n), sentinel, dtype=torch.float64, device=DEV)
        assert nh.lib().nfisam_factor_graph_hvp(ptr(dev["terms"]), nt, ptr(St), ptr(Vt), total, n, ptr(dev["slot_off"]), ns,
                                                ptr(dev["row_off"]), ptr(dev["row_slot"]), ptr(Ht), ptr(Gt) if score else null,
                                                ptr(scratch), null) == nh.OK
        torch.cuda.synchronize()
        return Ht.cpu().numpy(), Gt.cpu().numpy(), scratch.cpu().numpy()

    H2, G2, s2 = hvp(good, 10, True)
    H, G, s = hvp(terms, 10, True)
    assert not H.any() and not H2.any() and not G.any() and not G2.any()       # empty row lists: all zero
    for base, base2 in ((0, 0), (100, 20)):                                    # the slots of H v, then those of the score
        a, a2 = s[base:base + 100], s2[base2:base2 + 20]
        assert np.all(np.abs(a2[:4]) < 1e6) and np.all(np.abs(a2[10:12]) < 1e6)      # finite, and no sentinel was read
        assert np.array_equal(a[0:4], a2[0:4]) and np.array_equal(a[90:92], a2[10:12])
        assert np.all(a[4:10] == sentinel) and np.all(a[92:] == sentinel)
        for i, cnt in enumerate(owned, start=1):
            assert np.all(np.isnan(a[10 * i:10 * i + cnt])), i
            assert np.all(a[10 * i + cnt:10 * (i + 1)] == sentinel), i
    H3, G3, s3 = hvp(terms, 10, False)
    assert np.array_equal(s3, s[:100], equal_nan=True) and np.all(G3 == sentinel)     # without a score: Gt is not touched


def test_c_entry_refusals_and_empty_inputs():
    terms, gather, x, _, _, _ = _ksd_table()
    total, n, nt, ns = 13, 5, int(terms.shape[0]), int(gather["n_slots"])
    ptr, null = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(0)
    dev = nh._upload_named(DEV, terms=nh._table_bytes(terms), slot_off=gather["slot_off"], row_off=gather["row_off"],
                           row_slot=gather["row_slot"])
    St, Vt = _t(x[:n].T, np.float32), torch.ones(total, n, dtype=torch.float64, device=DEV)
    Ht = torch.full((total, n), 7.0, dtype=torch.float64, device=DEV)
    Gt = torch.full((total, n), 7.0, dtype=torch.float64, device=DEV)
    scratch = torch.zeros(2 * ns, n, dtype=torch.float64, device=DEV)
    entry, count = nh.lib().nfisam_factor_graph_hvp, nh.lib().nfisam_factor_graph_hvp_scratch_count

    def call(terms_=None, nt_=nt, St_=None, Vt_=None, total_=total, n_=n, so=None, ns_=ns, ro=None, rs=None, Ht_=None, sc=None):
        pick = lambda given, default: default if given is None else given
        return entry(pick(terms_, ptr(dev["terms"])), nt_, pick(St_, ptr(St)), pick(Vt_, ptr(Vt)), total_, n_,
                     pick(so, ptr(dev["slot_off"])), ns_, pick(ro, ptr(dev["row_off"])), pick(rs, ptr(dev["row_slot"])),
                     pick(Ht_, ptr(Ht)), ptr(Gt), pick(sc, ptr(scratch)), null)
    for bad in (dict(St_=null), dict(Vt_=null), dict(Ht_=null), dict(terms_=null), dict(so=null), dict(ro=null), dict(rs=null),
                dict(sc=null), dict(nt_=-1), dict(n_=-1), dict(total_=0), dict(total_=65536), dict(ns_=-1), dict(ns_=10 * nt + 1)):
        assert call(**bad) == nh.ERR_ARG, bad
    assert count(-1, 4, 0) == 0 and count(3, -1, 1) == 0 and count(3, 4, 0) == 12 and count(3, 4, 1) == 24
    torch.cuda.synchronize()
    assert bool((Ht == 7.0).all()) and bool((Gt == 7.0).all())                    # a refusal writes nothing
    assert call(n_=0) == nh.OK                                                   # no points: nothing is done
    torch.cuda.synchronize()
    assert bool((Ht == 7.0).all())
    assert call(nt_=0, terms_=null, so=null, ro=null, rs=null, sc=null, ns_=0) == nh.OK      # no terms: a zero product and score
    torch.cuda.synchronize()
    assert not Ht.any() and not Gt.any()
    none = np.zeros(0, dtype=nh.FACTOR_DTYPE)
    H0, G0 = nh.factor_graph_hvp_t(none, St, Vt, DEV, score=True)
    assert not H0.any() and not G0.any() and tuple(H0.shape) == (total, n)
    E = nh.factor_graph_hvp_t(terms, St[:, :0].contiguous(), Vt[:, :0].contiguous(), DEV, gather=gather)
    assert tuple(E.shape) == (total, 0)


# ---- 6. a quadratic graph: one Newton step, the Laplace blocks -------------------------------------------------------------------------------
def test_quadratic_graph_one_newton_step_and_the_laplace_blocks():
    """Three R2 landmarks, Gaussian priors and relative Gaussians only: log p is quadratic, H constant and -H positive definite."""
    L = [R2Variable("L%d" % i, VariableType.Landmark) for i in range(3)]
    rng = np.random.RandomState(21)

    def cov():
        q, _ = np.linalg.qr(rng.randn(2, 2))
        return (q * rng.uniform(0.05, 0.5, 2)) @ q.T
    factors = [F.UnaryR2GaussianPriorFactor(L[0], np.array([3.0, -40.0]), cov()),
               F.UnaryR2GaussianPriorFactor(L[2], np.array([25.0, 8.0]), cov()),
               F.R2RelativeGaussianLikelihoodFactor(L[0], L[1], np.array([10.0, 20.0]), cov()),
               F.R2RelativeGaussianLikelihoodFactor(L[1], L[2], np.array([12.0, 27.0]), cov())]
    col = {v: 2 * i for i, v in enumerate(L)}
    terms = nh.pack_factor_terms(factors, col)
    gather = nh.pack_score_gather(terms, 6)
    A, g0 = np.zeros((6, 6)), np.zeros(6)
    for f in factors:                                                            # host: -H and the score at the origin
        cols = _columns(f, col)
        A[np.ix_(cols, cols)] -= f.hess_x_log_pdf(np.zeros((1, cols.size)))[0]
        g0[cols] += f.grad_x_log_pdf(np.zeros((1, cols.size)))[0]
    star = np.linalg.solve(A, g0)
    cond, rtol, n = np.linalg.cond(A), 1e-12, 65
    Xt = _t(star[:, None] + rng.randn(6, n) * 3.0, np.float32)
    start = Xt.clone()

    def score_hvp(X, V):
        return nh.factor_graph_hvp_t(terms, X, V, DEV, gather=gather, score=True)

    def log_p(X):
        return nh.factor_graph_log_density_t(terms, X, DEV)
    spacing = 2.0 ** -23 * np.maximum(np.abs(star), 1.0)
    # the floor of the score next to the mode: |H| times the distance the stored point may lie from it (below)
    reach = spacing + cond * rtol * np.abs(start.cpu().numpy().astype(np.float64) - star[:, None]).max()
    out = ST.newton_refine_t(Xt, score_hvp, log_p, 1, rtol=rtol, gtol=float((np.abs(A) @ reach).max()))
    # the step is float64 and the point float32: one float32 spacing of the coordinate, plus what CG's rtol leaves of |d|
    d = np.abs(start.cpu().numpy().astype(np.float64) - star[:, None])
    err = np.abs(Xt.cpu().numpy().astype(np.float64) - star[:, None])
    assert np.all(err <= spacing[:, None] + cond * rtol * np.linalg.norm(d, axis=0)[None, :]), float((err / spacing[:, None]).max())
    assert out["steps"] == 1 and bool(out["converged"].all()) and not bool(out["negative_curvature"].any())
    assert bool((out["log_p"] > out["start_log_p"]).all()) and torch.equal(out["log_p"], log_p(Xt))
    # the Laplace blocks: every column of (-H)^-1 from ONE batched CG at the replicated point
    rtol = 1e-10
    rep = Xt[:, :1].expand(6, 6).contiguous()
    cg = ST.conjugate_gradient_t(lambda V: nh.factor_graph_hvp_t(terms, rep, V, DEV, gather=gather),
                                 torch.eye(6, dtype=torch.float64, device=DEV), 6, rtol)
    inv = np.linalg.inv(A)
    assert float(cg["residual"].max()) <= rtol and not bool(cg["negative_curvature"].any())
    assert np.abs(cg["x"].cpu().numpy() - inv).max() <= cond * rtol * np.linalg.norm(inv, 2)
    assert int(cg["iters"].max()) <= 6


# ---- 7. the solver -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_range(tmp_path_factory):
    """The small range problem through its six updates, once for the tests below: (solver, the last update's samples,
    arguments): the recipe of tests/test_sample_svgd_gpu.py, trained with the fixture's own arguments, unchanged."""
    from slam.NFiSAM import NFiSAM, NFiSAMArgs
    from slam.RunBatch import graph_file_parser, group_nodes_factors_incrementally
    fx = np.load(os.path.join(GOLDEN, "pipeline_small_range.npz"), allow_pickle=False)
    kwargs = json.loads(str(fx["arguments"]))
    kwargs["cuda_training"] = True
    path = tmp_path_factory.mktemp("small_range") / "factor_graph.fg"
    path.write_text(str(np.load(os.path.join(GOLDEN, "small_range_case1.npz"))["factor_graph_fg"]))
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    nodes, truth, factors = graph_file_parser(str(path), "fg", prior_cov_scale=0.1)
    steps = group_nodes_factors_incrementally(nodes, factors, incremental_step=int(fx["incremental_step"]))
    solver = NFiSAM(NFiSAMArgs(**kwargs))
    for vs, fs in steps:
        for v in vs: solver.add_node(v)
        for f in fs: solver.add_factor(f)
        solver.update_physical_and_working_graphs()
        smp = solver.incremental_inference()
    return solver, {v: np.array(smp[v]) for v in solver.elimination_ordering}, kwargs


def _state(solver):
    return (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
            list(solver.elimination_ordering), len(solver.physical_factors))


def _same_state(solver, state):
    return (torch.equal(state[0], torch.get_rng_state()) and torch.equal(state[1], torch.cuda.get_rng_state())
            and np.array_equal(state[2], np.random.get_state()[1]) and state[3] == random.getstate()
            and state[4] == list(solver.elimination_ordering) and state[5] == len(solver.physical_factors))


def test_small_range_joint_hessian_product(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    pcol, total = solver._post_columns()
    n = len(smp[order[0]])
    rng = np.random.RandomState(2)
    U, V = rng.randn(n, total), rng.randn(n, total)
    state = _state(solver)
    Hv = solver.joint_hessian_product(smp, V)
    Hu = solver.joint_hessian_product(smp, {v: U[:, pcol[v]:pcol[v] + v.dim] for v in order})
    assert Hv.shape == Hu.shape == (n, total) and Hv.dtype == np.float64 and np.all(np.isfinite(Hv)) and np.all(np.isfinite(Hu))
    assert np.array_equal(Hv, solver.joint_hessian_product(smp, V)) and _same_state(solver, state)
    # H is symmetric: u'(H v) = v'(H u) within the summed bound of the two products.  Per factor block the product's bound is
    # sum |H_rc| |v_c| (the fixture's rule); |H| |v| is not at hand matrix-free, so it is bounded by the host formulas' blocks
    x = np.zeros((n, total))
    for v in order:
        x[:, pcol[v]:pcol[v] + v.dim] = smp[v].astype(np.float32)
    bound = np.zeros(n)
    for f in solver.physical_factors:
        cols = np.concatenate([np.arange(pcol[v], pcol[v] + v.dim) for v in f.vars])
        absH = np.abs(f.hess_x_log_pdf(x[:, cols]))
        bound += np.einsum("nr,nrc,nc->n", np.abs(U[:, cols]), absH, np.abs(V[:, cols]))
    lhs, rhs = (U * Hv).sum(1), (V * Hu).sum(1)
    assert np.all(np.abs(lhs - rhs) <= 2.0 * C * EPS * bound), float((np.abs(lhs - rhs) / (EPS * bound)).max())
    for bad in (V[:, :-1], V[:-1], V[0], {v: U[:, pcol[v]:pcol[v] + v.dim] for v in order[1:]},
                {v: U[:-1, pcol[v]:pcol[v] + v.dim] for v in order}):
        with pytest.raises(ValueError, match="joint_hessian_product"):
            solver.joint_hessian_product(smp, bad)
    with pytest.raises(ValueError, match="joint_hessian_product"):
        solver.joint_hessian_product({}, V)


def test_small_range_map_newton(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    start = solver.joint_log_pdf(smp).max()
    state = _state(solver)
    launches = {"n": 0}
    names = ("_hvp_launch", "_joint_launch", "_score_launch")
    for name in names:                                                           # count the launches of the three fronts
        def counted(*a, _f=getattr(solver, name), **k):
            launches["n"] += 1
            return _f(*a, **k)
        setattr(solver, name, counted)
    try:
        out = solver.map_newton(smp)
        newton_launches, launches["n"] = launches["n"], 0
        ref = solver.map_refine(smp, steps=20)
        refine_launches = launches["n"]
    finally:
        for name in names:
            delattr(solver, name)
    assert set(out) == {"map_sample", "log_p", "start_log_p", "improved", "climbers", "steps", "grad_norm", "converged",
                        "negative_curvature", "top", "n"}
    assert out["start_log_p"] == start and out["log_p"] >= out["start_log_p"]
    assert out["improved"] == (out["log_p"] > out["start_log_p"]) and isinstance(out["improved"], bool)
    assert out["climbers"].shape == (8,) and out["climbers"].max() == out["log_p"] and out["top"] == 8
    assert out["grad_norm"].shape == out["converged"].shape == out["negative_curvature"].shape == (8,)
    assert out["converged"].dtype == out["negative_curvature"].dtype == np.bool_ and 0 <= out["steps"] <= 20
    assert np.array_equal(out["converged"], out["grad_norm"] <= ST.NEWTON_GTOL) and out["n"] == len(smp[order[0]])
    assert all(out["map_sample"][v].shape == (v.dim,) and out["map_sample"][v].dtype == np.float32 for v in order)
    again = solver.joint_log_pdf({v: out["map_sample"][v][None, :] for v in order})
    assert again.shape == (1,) and again[0] == out["log_p"]
    # not asserted against each other: nobody has measured which is higher on this problem
    print("map_newton: log p %.6f -> %.6f in %d steps, %d launches (converged %d of 8, negative curvature %d, grad norm %.3g);"
          " map_refine(steps=20): log p %.6f, %d launches"
          % (out["start_log_p"], out["log_p"], out["steps"], newton_launches, int(out["converged"].sum()),
             int(out["negative_curvature"].sum()), float(out["grad_norm"].min()), ref["log_p"], refine_launches))
    twice = solver.map_newton(smp)
    assert twice["log_p"] == out["log_p"] and np.array_equal(twice["climbers"], out["climbers"])
    assert all(np.array_equal(twice["map_sample"][v], out["map_sample"][v]) for v in order)
    assert np.array_equal(twice["grad_norm"], out["grad_norm"])
    still = solver.map_newton(smp, steps=0, top=3)
    assert still["log_p"] == start and not still["improved"] and still["climbers"].shape == (3,) and still["steps"] == 0
    best = solver.map_estimate(smp)
    assert all(np.array_equal(still["map_sample"][v], np.asarray(best[v], dtype=np.float32)) for v in order)
    assert _same_state(solver, state)
    for bad in (dict(top=0), dict(top=1.5), dict(steps=-1), dict(rtol=0), dict(damping=-1), dict(cg_iters=0), dict(gtol=0.0),
                dict(backtracks=-1)):
        with pytest.raises(ValueError, match="map_newton"):
            solver.map_newton(smp, **bad)
    with pytest.raises(ValueError, match="map_newton"):
        solver.map_newton({})


def test_small_range_laplace_approximation(small_range):
    solver, smp, kwargs = small_range
    order = solver.elimination_ordering
    state = _state(solver)
    out = solver.laplace_approximation(samples=smp, pairs=[(order[0], order[1])])
    assert set(out) == {"point", "log_p", "cov", "pair_cov", "residual", "negative_curvature"}
    assert isinstance(out["negative_curvature"], bool) and isinstance(out["residual"], float) and np.isfinite(out["log_p"])
    assert set(out["cov"]) == set(order) and set(out["pair_cov"]) == {(order[0], order[1])}
    blocks = [(v.dim, out["cov"][v]) for v in order] + [(order[0].dim + order[1].dim, out["pair_cov"][(order[0], order[1])])]
    for d, b in blocks:
        assert b.shape == (d, d) and b.dtype == np.float64 and np.array_equal(b, b.T) and np.all(np.isfinite(b))
        if not out["negative_curvature"]:
            assert np.linalg.eigvalsh(b).min() > 0
    print("laplace_approximation: log p %.6f, residual %.3g, negative curvature %s, position sigmas %s"
          % (out["log_p"], out["residual"], out["negative_curvature"],
             ", ".join("%s %.3g" % (v.name, float(np.sqrt(abs(out["cov"][v][0, 0])))) for v in order)))
    newton = solver.map_newton(smp)
    assert out["log_p"] == newton["log_p"] and all(np.array_equal(out["point"][v], newton["map_sample"][v]) for v in order)
    at = solver.laplace_approximation(point=newton["map_sample"], variables=[order[0]])
    assert set(at["cov"]) == {order[0]} and at["pair_cov"] == {} and at["cov"][order[0]].shape == (order[0].dim,) * 2
    assert at["log_p"] == out["log_p"] and np.array_equal(at["cov"][order[0]], at["cov"][order[0]].T)
    assert _same_state(solver, state)
    short = dict(newton["map_sample"])
    short[order[0]] = np.zeros(order[0].dim + 1)
    for bad in (dict(point=short), dict(point=newton["map_sample"], max_columns=2), dict(point=newton["map_sample"], rtol=0),
                dict(point=newton["map_sample"], cg_iters=0), dict(point=newton["map_sample"], pairs=[(order[0],)]),
                dict(point=newton["map_sample"], variables=[]), dict(point=newton["map_sample"], steps=3), dict(samples=smp, top=0)):
        with pytest.raises(ValueError, match="laplace_approximation|map_newton"):
            solver.laplace_approximation(**bad)
