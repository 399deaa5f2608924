"""The posterior log-density surface without a GPU: the C entry is declared and exported, the binding and
`NFiSAM.posterior_log_pdf` exist, and bad input is refused with the documented errors BEFORE anything is launched."""
import os
import re

import numpy as np
import pytest

import nfisam_hip as nh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_the_binding_exports_it():
    hdr = open(os.path.join(ROOT, "include", "nfisam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+nfisam_nsf_posterior_log_density\s*\(([^)]*)\)", hdr)
    assert m is not None
    params = [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["table", "n_cliques", "cols", "obs", "max_D", "K", "H", "B", "L", "n", "St", "log_q", "per_clique",
                      "latent", "stream"]
    assert "nfisam_nsf_posterior_log_density" in nh.EXPORTS
    nh.build()
    assert hasattr(nh.lib(), "nfisam_nsf_posterior_log_density")
    assert nh.lib().nfisam_abi_version() == 1600          # additive entry: the ABI version stays


def test_binding_and_solver_method_exist():
    from slam.NFiSAM import NFiSAM
    from slam.ParallelNFiSAM import ParallelNFiSAM
    assert callable(nh.posterior_log_density)
    assert callable(NFiSAM.posterior_log_pdf)
    assert ParallelNFiSAM.posterior_log_pdf is NFiSAM.posterior_log_pdf


def _one_clique_table(D=5, n_obs=1, n_sep=2, n_frontal=2):
    t = np.zeros(1, dtype=nh.POST_DTYPE)
    t["D_model"], t["n_obs"], t["n_sep"], t["n_frontal"] = D, n_obs, n_sep, n_frontal
    t["obs_off"], t["sep_off"], t["front_off"] = 0, 0, n_sep
    return t


def test_binding_refuses_bad_tables_before_any_launch():
    nh.build()
    S = np.zeros((10, 4), dtype=np.float32)
    t = _one_clique_table()
    obs = np.zeros(1, dtype=np.float32)
    with pytest.raises(ValueError, match="out of range"):
        nh.posterior_log_density(t, np.array([0, 1, 2, 4], dtype=np.int32), obs, S, 5, 9, 8, 5.0, 1, "cpu")
    with pytest.raises(ValueError, match="out of range"):
        nh.posterior_log_density(t, np.array([0, -1, 2, 3], dtype=np.int32), obs, S, 5, 9, 8, 5.0, 1, "cpu")
    with pytest.raises(ValueError):                        # unsupported (K, H)
        nh.posterior_log_density(t, np.array([0, 1, 2, 3], dtype=np.int32), obs, S, 5, 40, 8, 5.0, 1, "cpu")
    with pytest.raises(ValueError, match="max_D"):         # a model wider than the LDS rows the launch is sized for
        nh.posterior_log_density(t, np.array([0, 1, 2, 3], dtype=np.int32), obs, S, 4, 9, 8, 5.0, 1, "cpu")
    with pytest.raises(ValueError, match="offsets"):       # observations missing
        nh.posterior_log_density(t, np.array([0, 1, 2, 3], dtype=np.int32), obs[:0], S, 5, 9, 8, 5.0, 1, "cpu")
    with pytest.raises(ValueError, match="model dimension"):
        nh.posterior_log_density(_one_clique_table(D=4), np.array([0, 1, 2, 3], dtype=np.int32), obs, S, 5, 9, 8, 5.0, 1,
                                 "cpu")


class _Refuse:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("launched despite invalid input")


def _fake_tree_solver(monkeypatch):
    """A solver whose physical tree is one clique {X0, L1} with a (never used) model: enough to reach the argument checks."""
    from slam.BayesTree import BayesTree, BayesTreeNode
    from slam.NFiSAM import NFiSAM
    from slam.Variables import R2Variable, SE2Variable, VariableType
    X0, L1 = SE2Variable("X0"), R2Variable("L1", VariableType.Landmark)
    s = NFiSAM()
    root = BayesTreeNode(frontal={X0, L1})
    s._physical_bayes_tree = BayesTree(root_clique=root)
    s._clique_density_model[root] = object()
    s._elimination_ordering = [X0, L1]
    refuse = _Refuse()
    monkeypatch.setattr(nh, "posterior_log_density", refuse)
    monkeypatch.setattr(nh, "posterior_log_density_t", refuse)
    monkeypatch.setattr(NFiSAM, "_posterior_table", refuse)
    return s, X0, L1, refuse


def test_posterior_log_pdf_errors_come_before_any_launch(monkeypatch):
    from slam.NFiSAM import NFiSAM
    nh.build()
    with pytest.raises(RuntimeError, match="no Bayes tree"):
        NFiSAM().posterior_log_pdf({})
    s, X0, L1, refuse = _fake_tree_solver(monkeypatch)
    with pytest.raises(ValueError, match="L1"):
        s.posterior_log_pdf({X0: np.zeros((7, 3))})
    with pytest.raises(ValueError, match="ragged"):
        s.posterior_log_pdf({X0: np.zeros((7, 3)), L1: np.zeros((6, 2))})
    with pytest.raises(ValueError, match="X0"):            # wrong width
        s.posterior_log_pdf({X0: np.zeros((7, 2)), L1: np.zeros((7, 2))})
    assert refuse.calls == 0
    # a tree whose clique has no trained model yet
    s._clique_density_model.clear()
    with pytest.raises(RuntimeError, match="no trained model"):
        s.posterior_log_pdf({X0: np.zeros((7, 3)), L1: np.zeros((7, 2))})
    assert refuse.calls == 0
