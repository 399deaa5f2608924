"""The device's factor values and scores (nfisam_factor_graph_log_density, nfisam_factor_graph_score) against the 60-digit
values of tests/golden/factor_exact.npz, with the bound and the constant of tests/test_factor_exact_cpu.py:

    |device - exact| <= C x 2^-53 x scale + allow,   C = 256

(`scale`: the fixture's running error bound of the value; `allow`: w^2 / 12 where |w| < 1e-5 for a value, nothing for a score).
Only the .npz files are read.  One table per group, built like `_case_table` of tests/test_factor_density_gpu.py:
  * every case with one factor (part (a) of factor_density.npz, the range, ring, mixture and R2 edge cases), each in columns of
    its own, its points cycled to n = 80: one full 64-point tile and a partial one;
  * the SE(2) sweeps, where every point has an observation of its own: the factors of the four prior cases share one pose's
    rows, those of the three relative-pose cases two poses' rows, and factor i is graded at point i (n = 171 and 123);
  * the whole graphs through `pack_factor_terms` and `pack_score_gather`.
Graded: the per-factor terms and the totals of the density entry, the slots and the gathered rows of the score entry.  The largest
ratio |device - exact| / (2^-53 scale) per case is printed; the MI355X's are in profiles/factor_exact.json next to the host's
(largest: 3.8 on a value and 3.1 on a score over the cases, 5.8 on a term of Manhattan-136)."""
import numpy as np
import pytest
import torch

import nfisam_hip as nh
from factors import Factors as F
from test_factor_density_cpu import GRAPHS
from test_factor_density_gpu import _case_table
from test_factor_exact_cpu import C, exact_cases, exact_fixture, exact_graph, ratio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_SINGLE = 80


def _columns(f, r):
    return np.concatenate([np.arange(r[v], r[v] + v.dim) for v in f.vars])


def _report(name, cls, r_v, r_s):
    print("%-26s %-42s |device - exact| / (2^-53 scale): value %8.3g  score %8.3g" % (name, cls, r_v, r_s))


def test_single_factor_cases_terms_totals_slots_and_rows():
    cases = [c for c in exact_cases() if len(c.factors) == 1]
    assert len(cases) >= 28 + 15
    terms, rows, total = _case_table([(c.cls, c.factors[0], c.x, None) for c in cases])
    assert set(terms["code"]) == set(nh.FAC_CODES.values())                      # every device code is exercised
    n = N_SINGLE
    S = np.zeros((n, total), dtype=np.float32)
    for c, r in zip(cases, rows):
        S[:, _columns(c.factors[0], r)] = c.x[np.arange(n) % c.x.shape[0]]
    log_p, per = nh.factor_graph_log_density(terms, S, DEV, per_factor=True)
    G, slots = nh.factor_graph_score(terms, S, DEV, slots=True)
    assert per.dtype == G.dtype == slots.dtype == torch.float64
    log_p, per, G, slots = log_p.cpu().numpy(), per.cpu().numpy(), G.cpu().numpy(), slots.cpu().numpy()
    gather = nh.pack_score_gather(terms, total)
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(G)) and np.all(np.isfinite(slots))      # finite everywhere
    worst, tot, tot_scale, tot_allow = {}, np.zeros(n), np.zeros(n), np.zeros(n)
    for i, (c, r) in enumerate(zip(cases, rows)):
        idx = np.arange(n) % c.x.shape[0]
        m = c.mask[idx]
        got = G[:, _columns(c.factors[0], r)]
        r_v = ratio(per[i], c.logp[idx], c.logp_scale[idx], c.logp_allow[idx])
        r_s = ratio(got[m], c.score[idx][m], c.score_scale[idx][m])
        if not isinstance(c.factors[0], F.BinaryFactorMixture):
            assert np.all(got[~m] == 0.0), c.name                                # a range of exactly 0: the zero vector
        worst[c.name] = (r_v, r_s)
        _report(c.name, c.cls, r_v, r_s)
        tot, tot_scale, tot_allow = tot + c.logp[idx], tot_scale + c.logp_scale[idx], tot_allow + c.logp_allow[idx]
    # every gathered row is the left-to-right sum of its slots (one slot, or two where a candidate is listed twice): the graded
    # rows are the graded slots
    ro, rs = gather["row_off"], gather["row_slot"]
    assert slots.shape == (gather["n_slots"], n) and max(ro[r + 1] - ro[r] for r in range(total)) == 2
    for r in range(total):
        acc = np.zeros(n)
        for sl in rs[ro[r]:ro[r + 1]]:
            acc = acc + slots[sl]
        assert np.array_equal(G[:, r], acc), r
    r_t = ratio(log_p, tot, tot_scale, tot_allow)
    print("totals over %d cases: %.3g;  largest: value %.3g, score %.3g (C = %g)"
          % (len(cases), r_t, max(v for v, s in worst.values()), max(s for v, s in worst.values()), C))
    bad = {k: v for k, v in worst.items() if max(v) > C}
    assert not bad and r_t <= C, (bad, r_t)


@pytest.mark.parametrize("kind", ["se2_prior", "se2_rel"])
def test_se2_sweeps_one_observation_per_point(kind):
    """Every point of the sweeps has its own observation: all factors of a kind share the rows of one pose (two poses), the point
    of factor i is row i, and per_factor[i, i] / the slots of factor i at point i are graded.  Rows with |w| >= 1e-3 have no
    allowance: there the value the device matches and the score it matches are the density and the gradient of ONE function
    of one residual (the same bound, stated once more)."""
    cases = [c for c in exact_cases() if c.name.startswith(kind)]
    assert [c.name for c in cases][:3] == [kind + "_" + t for t in ("tight", "medium", "full")]
    width = cases[0].x.shape[1]
    factors = [f for c in cases for f in c.factors]
    terms = np.concatenate([nh.pack_factor_terms([f], {v: 3 * j for j, v in enumerate(f.vars)}) for f in factors])
    S = np.concatenate([c.x for c in cases])
    n = S.shape[0]
    assert n == len(factors) and 64 < n <= 192 and S.dtype == np.float32
    per = nh.factor_graph_log_density(terms, S, DEV, per_factor=True)[1].cpu().numpy()
    slots = nh.factor_graph_score(terms, S, DEV, slots=True)[1].cpu().numpy()
    slot_off = nh.pack_score_gather(terms, width)["slot_off"]
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(slots))
    value = np.diagonal(per)
    score = np.stack([slots[slot_off[i]:slot_off[i] + width, i] for i in range(n)])
    off, bad, same = 0, {}, 0
    for c in cases:
        m = c.x.shape[0]
        v, s = value[off:off + m], score[off:off + m]
        r_v, r_s = ratio(v, c.logp, c.logp_scale, c.logp_allow), ratio(s, c.score, c.score_scale)
        _report(c.name, c.cls, r_v, r_s)
        if max(r_v, r_s) > C:
            bad[c.name] = (r_v, r_s)
        big = np.abs(c.w) >= 1e-3
        assert not c.logp_allow[big].any() and big.sum() >= 15
        assert ratio(v[big], c.logp[big], c.logp_scale[big]) <= C and ratio(s[big], c.score[big], c.score_scale[big]) <= C, c.name
        same += int(big.sum())
        off += m
    assert not bad, bad
    assert same >= 45


def test_part_a_se2_rows_with_a_large_residual_see_one_function():
    cases = [c for c in exact_cases() if c.w is not None and len(c.factors) == 1]
    assert len(cases) == 8
    terms, rows, total = _case_table([(c.cls, c.factors[0], c.x, None) for c in cases])
    S = np.zeros((32, total), dtype=np.float32)
    for c, r in zip(cases, rows):
        S[:, _columns(c.factors[0], r)] = c.x
    per = nh.factor_graph_log_density(terms, S, DEV, per_factor=True)[1].cpu().numpy()
    G = nh.factor_graph_score(terms, S, DEV).cpu().numpy()
    same = 0
    for i, (c, r) in enumerate(zip(cases, rows)):
        big = np.abs(c.w) >= 1e-3
        assert not c.logp_allow[big].any()
        got = G[:, _columns(c.factors[0], r)]
        assert ratio(per[i][big], c.logp[big], c.logp_scale[big]) <= C, c.name
        assert ratio(got[big], c.score[big], c.score_scale[big]) <= C, c.name
        same += int(big.sum())
    assert same >= 150                                                          # (the tight prior's headings are mostly closer)


@pytest.mark.parametrize("key", sorted(GRAPHS) + ["ksd"])
def test_whole_graphs_through_the_packers(key):
    fx = exact_fixture()
    factors, col, x, ex = exact_graph(fx, key)
    terms = nh.pack_factor_terms(factors, col)
    gather = nh.pack_score_gather(terms, x.shape[1])
    log_p, per = nh.factor_graph_log_density(terms, x, DEV, per_factor=True)
    G = nh.factor_graph_score(terms, x, DEV, gather=gather)
    log_p, per, G = log_p.cpu().numpy(), per.cpu().numpy(), G.cpu().numpy()
    r = (ratio(per, ex["terms"], ex["terms_scale"], ex["terms_allow"]), ratio(log_p, ex["total"], ex["total_scale"], ex["total_allow"]),
         ratio(G, ex["score"], ex["score_scale"]))
    print("%s: %d factors x %d points: |device - exact| / (2^-53 scale): terms %.3g, totals %.3g, joint score %.3g"
          % (key, len(factors), x.shape[0], *r))
    assert max(r) <= C, r
