"""The score of the joint density on the GPU (nfisam_factor_graph_score, nfisam_hip.factor_graph_score, NFiSAM.joint_score)
against tests/golden/factor_score.npz and against the host `Factors.grad_x_log_pdf`, plus the fixed summation order, bitwise
repeatability and the conventions at a range of 0 and far from every mixture component.

Bounds, |device - yardstick| <= TOL (|yardstick| + 1), each 16 x the largest deviation measured on the MI355X over the
values it covers (DEVICE_MEASURED below, recorded in profiles/ksd.json):
  * against the fixture, every value of part (a) / of the whole graphs: 0.301 / 1.95e-3 -- the same figures as the host
    formulas on the CPU (tests/test_factor_score_cpu.py: they are the REFERENCE's cancellation in its SE(2) gradient, not the
    device's error), and far below 100 x them;
  * against the fixture where the reference does not cancel: ranges and mixtures 5.2e-16, the three R2 classes (Richardson
    differences) 7.3e-11, SE(2) rows with |w| >= 1e-3 4.4e-7 -- again the host's figures (3.8e-16, 7.3e-11, 4.4e-7);
  * against the host `grad_x_log_pdf` at the same float32 points (both the derivative of the same smooth float64 formula,
    with the same series switch): 6.5e-14 on part (a) (an SE(2) relative-pose case), 1.9e-13 on the whole graphs (sums of up
    to 429 terms per row on Plaza1-ADA)."""
import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from slam.Variables import R2Variable, SE2Variable, VariableType
from test_factor_density_cpu import GRAPHS
from test_factor_density_gpu import _case_points, _case_table
from test_factor_score_cpu import (deviation, graph_scores, heading_residual, host_joint_score, ksd_graph, part_a_scores,
                                   score_fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# largest |device - yardstick| / (|yardstick| + 1) measured on the MI355X
DEVICE_MEASURED = {"part_a": 0.301, "graphs": 1.95e-3, "exact": 5.3e-16, "fd": 7.4e-11, "se2": 4.5e-7,
                   "host": 6.6e-14, "host_graphs": 1.9e-13}
TOL = {k: 16 * v for k, v in DEVICE_MEASURED.items()}
NS = (1, 63, 64, 65, 130)


def _cases():
    """part (a) in the form `_case_table` of the density tests takes, and the score side of it."""
    scores = part_a_scores()
    return [(cls, f, x, None) for cls, f, x, ref, mask, group in scores], scores


def _case_columns(f, r):
    return np.concatenate([np.arange(r[v], r[v] + v.dim) for v in f.vars])


@pytest.mark.parametrize("n", NS)
def test_every_code_matches_the_fixture_and_the_host_formulas(n):
    cases, scores = _cases()
    terms, rows, total = _case_table(cases)
    assert set(terms["code"]) == set(nh.FAC_CODES.values())                 # every device code is exercised
    S = np.zeros((n, total + 2), dtype=np.float32)                          # two rows at the end that no factor touches
    for (cls, f, x, _), r in zip(cases, rows):
        idx, off = np.arange(n) % x.shape[0], 0
        for v in f.vars:
            S[:, r[v]:r[v] + v.dim] = x[idx, off:off + v.dim]
            off += v.dim
    G = nh.factor_graph_score(terms, S, DEV)
    assert G.dtype == torch.float64 and tuple(G.shape) == (n, total + 2)
    G = G.cpu().numpy()
    assert np.all(np.isfinite(G)) and np.all(G[:, total:] == 0.0)            # a row without a factor is exactly 0
    worst = dict(part_a=0.0, exact=0.0, fd=0.0, se2=0.0, host=0.0)
    for (cls, f, x, ref, mask, group), r in zip(scores, rows):
        idx = np.arange(n) % x.shape[0]
        got, m = G[:, _case_columns(f, r)], mask[idx]
        host = f.grad_x_log_pdf(x[idx].astype(np.float64))
        d_all, d_host = deviation(got[m], ref[idx][m]), deviation(got, host)
        if group == "se2":
            big = np.abs(heading_residual(f, x[idx])) >= 1e-3
            d = deviation(got[big], ref[idx][big])
        else:
            d = d_all
            if cls != "AmbiguousDataAssociationFactor":
                assert np.all(got[~m] == 0.0), cls                           # a range of exactly 0: the zero vector
        print("n = %3d  %-42s |device - ref| / (|ref| + 1): all %.3g, %s %.3g;  vs host %.3g" % (n, cls, d_all, group, d, d_host))
        worst["part_a"], worst[group], worst["host"] = max(worst["part_a"], d_all), max(worst[group], d), max(worst["host"], d_host)
    print("n = %3d  measured:" % n, worst)
    assert all(worst[k] <= TOL[k] for k in worst), worst


def _graph(key):
    factors, col, x, ref = graph_scores(key)
    return nh.pack_factor_terms(factors, col), factors, col, x, ref


@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_whole_graph_scores_order_and_bits(key):
    terms, factors, col, x, ref = _graph(key)
    total = x.shape[1]
    gather = nh.pack_score_gather(terms, total)
    G, slots = nh.factor_graph_score(terms, x, DEV, slots=True)
    G, slots = G.cpu().numpy(), slots.cpu().numpy()
    d_ref, d_host = deviation(G, ref), deviation(G, host_joint_score(factors, col, x))
    print("%s: %d factors x %d points: |device - ref| / (|ref| + 1) = %.3g, vs host %.3g" % (key, len(factors), x.shape[0],
                                                                                            d_ref, d_host))
    assert d_ref <= TOL["graphs"] and d_host <= TOL["host_graphs"]
    # the documented order: every row is the left-to-right float64 sum of its slots in table order, exactly
    assert slots.shape == (gather["n_slots"], x.shape[0]) and np.all(np.isfinite(slots))
    want = np.zeros((x.shape[0], total))
    ro, rs = gather["row_off"], gather["row_slot"]
    for r in range(total):
        acc = np.zeros(x.shape[0])
        for s in rs[ro[r]:ro[r + 1]]:
            acc = acc + slots[s]
        want[:, r] = acc
    assert np.array_equal(G, want)
    assert max(ro[r + 1] - ro[r] for r in range(total)) >= (3 if key == "manhattan136" else 100)   # rows many factors share
    # a second call, from a device tensor and with the lists reused: the same bits
    again = nh.factor_graph_score(terms, torch.from_numpy(x).to(DEV), DEV, gather=gather).cpu().numpy()
    assert np.array_equal(again, G)
    # a point's column does not depend on n or on its tile: the same points cycled to n = 65 and n = 130
    g65 = nh.factor_graph_score(terms, x[np.arange(65) % x.shape[0]], DEV, gather=gather).cpu().numpy()
    g130 = nh.factor_graph_score(terms, x[np.arange(130) % x.shape[0]], DEV, gather=gather).cpu().numpy()
    assert np.array_equal(g130[:65], g65) and np.array_equal(g130[64], g65[64])
    assert np.array_equal(g130[:x.shape[0]], G) and np.array_equal(g130[65:65 + 3], g130[np.arange(65, 68) % x.shape[0]])


def test_the_ksd_graph_and_a_twice_listed_candidate():
    fs = score_fixture()
    variables, factors = ksd_graph(fs["ksd_truth"])
    X2, L0 = variables[2], variables[3]
    factors = factors + [F.BinaryFactorWithNullHypo(X2, L0, np.array([0.8, 0.2]), F.SE2R2RangeGaussianLikelihoodFactor, 3.2,
                                                    0.3, 6.0)]
    col, off = {}, 0
    for v in variables:
        col[v] = off
        off += v.dim
    terms = nh.pack_factor_terms(factors, col)
    assert terms["k"][-1] == 2 and terms["cand"][-1, 0] == terms["cand"][-1, 1] == col[L0]
    x = fs["ksd_samples"]
    G = nh.factor_graph_score(terms, x, DEV).cpu().numpy()
    assert deviation(G, host_joint_score(factors, col, x)) <= TOL["host_graphs"]
    G0 = nh.factor_graph_score(terms[:-1], x, DEV).cpu().numpy()
    assert deviation(G0, fs["ksd_score"]) <= TOL["graphs"]
    extra = factors[-1].grad_x_log_pdf(np.concatenate([x[:, 6:9], x[:, 9:11]], 1).astype(np.float64))
    assert deviation((G - G0)[:, 9:11], extra[:, 3:]) <= 1e-9                # both components landed in L0's two rows


def test_range_zero_is_zero_and_far_mixtures_are_finite():
    X = SE2Variable("X0")
    L = [R2Variable("L%d" % i, VariableType.Landmark) for i in range(2)]
    factors = [F.SE2R2RangeGaussianLikelihoodFactor(X, L[0], 4.0, 0.5),
               F.UnaryR2RangeGaussianPriorFactor(L[1], np.array([1.0, -2.0]), 3.0, 0.4),
               F.AmbiguousDataAssociationFactor(X, L, np.array([0.3, 0.7]), F.SE2R2RangeGaussianLikelihoodFactor, 5.0, 0.4)]
    col = {X: 0, L[0]: 3, L[1]: 5}
    terms = nh.pack_factor_terms(factors, col)
    S = np.zeros((66, 7), dtype=np.float32)
    S[:, :3] = [2.0, 3.0, 0.5]
    S[:, 3:5] = [2.0, 3.0]                                                    # L0 on the pose: range 0 (and in the mixture)
    S[:, 5:7] = [1.0, -2.0]                                                   # L1 on its ring's centre: range 0
    G, slots = nh.factor_graph_score(terms, S, DEV, slots=True)
    slots = slots.cpu().numpy()
    assert np.all(np.isfinite(G.cpu().numpy()))
    assert np.all(slots[:4] == 0.0) and np.all(slots[4:6] == 0.0)             # the range factor and the ring prior
    far = S.copy()
    far[:, 3:] += 1.0e4                                                       # every candidate 1e4 m away
    G = nh.factor_graph_score(terms, far, DEV).cpu().numpy()
    assert np.all(np.isfinite(G)) and np.abs(G).max() > 1e3
    assert deviation(G, host_joint_score(factors, col, far)) <= TOL["host"]


def test_empty_inputs_and_the_c_entry_refusals():
    import ctypes as C
    terms, factors, col, x, ref = _graph("manhattan136")
    assert tuple(nh.factor_graph_score(terms, x[:0], DEV).shape) == (0, x.shape[1])
    z = nh.factor_graph_score(terms[:0], x, DEV)
    assert z.dtype == torch.float64 and not z.cpu().numpy().any()
    St = torch.zeros(4, 8, dtype=torch.float32, device=DEV)
    Gt = torch.zeros(4, 8, dtype=torch.float64, device=DEV)
    tb = torch.zeros(160, dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(8, dtype=torch.int32, device=DEV)
    scr = torch.zeros(80, dtype=torch.float64, device=DEV)
    call, null = nh.lib().nfisam_factor_graph_score, C.c_void_p(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    ok = (ptr(tb), 1, ptr(St), 4, 8, ptr(i32), 0, ptr(i32), ptr(i32), ptr(Gt), ptr(scr), null)
    for k, bad in ((0, null), (2, null), (5, null), (7, null), (8, null), (9, null), (10, null), (1, -1), (3, 0), (4, -8),
                   (6, -1), (6, 11), (3, 65536)):
        args = list(ok)
        args[k] = bad
        assert call(*args) == nh.ERR_ARG, k
    # a zeroed record has code 0: no slot, every row has an empty list -> zeros, nothing read or written out of bounds
    assert call(*ok) == nh.OK
    torch.cuda.synchronize()
    assert not Gt.cpu().numpy().any()


def test_one_guard_serves_both_entries():
    """Ten records in two FAC_RUN runs, eight of them bad, straight into both C entries (the Python checks refuse each of them):
    a bad record reads nothing -- St is the middle of a larger tensor whose outer rows hold a sentinel no result may show --
    and yields NaN as its term and in the slots it owns; the good records' bits are those of the table without the bad ones."""
    import ctypes as C
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
    for t in bad:                                                             # before any launch: each refused on its own
        with pytest.raises(ValueError):
            nh.check_factor_terms(t, total)
    terms = np.concatenate([good[:1]] + bad + [good[1:]])
    assert terms.shape[0] == 10 and nh.check_factor_terms(good, total) is None
    rng = np.random.RandomState(3)
    big = torch.full((11, n), sentinel, dtype=torch.float32, device=DEV)
    big[2:9] = torch.from_numpy((rng.randn(total, n) * 2.0).astype(np.float32)).to(DEV)
    St = big[2:9]
    assert St.is_contiguous()
    ptr, null = (lambda t: C.c_void_p(t.data_ptr())), C.c_void_p(0)

    def density(tb):
        dev, = nh.upload(nh._table_bytes(tb), device=DEV)
        log_p = torch.zeros(n, dtype=torch.float64, device=DEV)
        per = torch.zeros(tb.shape[0], n, dtype=torch.float64, device=DEV)
        assert nh.lib().nfisam_factor_graph_log_density(ptr(dev), tb.shape[0], ptr(St), total, n, ptr(log_p), ptr(per), null) == nh.OK
        torch.cuda.synchronize()
        return log_p.cpu().numpy(), per.cpu().numpy()

    def score(tb, stride):
        nt, ns = tb.shape[0], stride * tb.shape[0]
        dev = nh._upload_named(DEV, terms=nh._table_bytes(tb), slot_off=stride * np.arange(nt, dtype=np.int32),
                               row_off=np.zeros(total + 1, dtype=np.int32), row_slot=np.zeros(1, dtype=np.int32))
        Gt = torch.full((total, n), sentinel, dtype=torch.float64, device=DEV)
        scratch = torch.full((ns, n), sentinel, dtype=torch.float64, device=DEV)
        assert nh.lib().nfisam_factor_graph_score(ptr(dev["terms"]), nt, ptr(St), total, n, ptr(dev["slot_off"]), ns,
                                                  ptr(dev["row_off"]), ptr(dev["row_slot"]), ptr(Gt), ptr(scratch), null) == nh.OK
        torch.cuda.synchronize()
        return Gt.cpu().numpy(), scratch.cpu().numpy()

    log_p2, per2 = density(good)
    log_p, per = density(terms)
    assert np.all(np.isfinite(per2)) and np.all(np.abs(per2) < 1e6)            # (no sentinel went into a good term)
    assert np.all(np.isnan(per[1:9])) and np.all(np.isnan(log_p))
    assert np.array_equal(per[0], per2[0]) and np.array_equal(per[9], per2[1])
    G2, s2 = score(good, 10)
    G, s = score(terms, 10)
    assert not G.any() and not G2.any()                                        # empty row lists: Gt is all zero
    assert np.all(np.isfinite(s2[:4])) and np.all(np.isfinite(s2[10:12])) and np.all(np.abs(s2[:4]) < 1e6)
    assert np.array_equal(s[0:4], s2[0:4]) and np.array_equal(s[90:92], s2[10:12])
    assert np.all(s[4:10] == sentinel) and np.all(s[92:] == sentinel)
    for i, cnt in enumerate(owned, start=1):
        assert np.all(np.isnan(s[10 * i:10 * i + cnt])), i
        assert np.all(s[10 * i + cnt:10 * (i + 1)] == sentinel), i
