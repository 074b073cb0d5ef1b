"""Deterministic pairwise fit, the parts that need no GPU: the two C
entries are declared and listed, and the ranker refuses the list objectives before any handle
exists."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spfm_psgd_pairs_set_deterministic", "spfm_psgd_pairs_get_deterministic")


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_declared_and_listed(name):
    from sparsepoly_amd import _capi

    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        assert re.search(r"^int %s\(spfm_handle h, " % name, f.read(), re.M)
    assert name in _capi.SYMBOLS


@pytest.mark.parametrize("objective", ["softmax", "list"])
def test_ranker_refuses_the_lists_and_only_them(objective, monkeypatch):
    from sparsepoly_amd import SparseFactorizationMachineRanker, pairwise

    def boom(self):
        raise RuntimeError("reached the engine")

    monkeypatch.setattr(pairwise._BaseSparseFactorizationMachine, "_new_engine", boom)
    X = sp.csr_matrix(np.eye(3, 6))
    Z = sp.csr_matrix(np.eye(3, 6, k=3))
    t = np.array([[0, 1, 2], [1, 0, 2]])
    est = SparseFactorizationMachineRanker(regularizer="l1")
    est.deterministic = True
    with pytest.raises(ValueError, match="lists"):
        est.fit(X, Z, triples=t, objective=objective)
    with pytest.raises(RuntimeError, match="reached the engine"):   # pairwise: no refusal
        est.fit(X, Z, triples=t)
