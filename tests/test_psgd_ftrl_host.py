"""FTRL-Proximal steps of the minibatch fits: what needs no device."""
import os
import re

import numpy as np
import pytest
from conftest import ROOT


def test_header_and_capi_declare_the_ftrl_entries():
    from sparsepoly_amd import _capi
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    for name in ("spfm_psgd_set_ftrl", "spfm_psgd_get_ftrl"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _capi.SYMBOLS


def test_squared_norm_is_refused_before_an_engine_exists(monkeypatch):
    import scipy.sparse as sp

    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd import engine as engine_mod
    monkeypatch.setattr(engine_mod.HipEngine, "__init__",
                        lambda *a, **k: pytest.fail("a device handle was requested"))
    Xs, y = sp.csr_matrix(np.random.RandomState(0).randn(12, 5)), np.arange(12.0)
    kw = dict(solver="psgd", learning_rate="ftrl", max_iter=1)
    with pytest.raises(ValueError, match="squaredl12 / squaredl21"):
        SparseFactorizationMachineRegressor(regularizer="squaredl12", **kw).fit(Xs, y)


@pytest.mark.parametrize("reg", ["l1", "l21"])
def test_closed_form_of_the_derived_start_is_the_start(reg):
    from sparsepoly_amd.pairwise import ftrl_closed_form, ftrl_start
    rng = np.random.RandomState(3)
    P, w = rng.randn(2, 5, 9), rng.randn(9)
    P[0, :, 4] = 0.0          # a zero column
    P[1, 2, :3] = 0.0         # zero components inside live columns
    G0, eta0, alpha, beta, gamma = 0.7, 0.05, 1e-2, 3e-2, 0.4
    z_P, z_w, n_P, n_w = ftrl_start(P, w, G0, eta0, alpha, beta, gamma, reg)
    assert not n_P.any() and not n_w.any() and not z_P[0, :, 4].any()
    P1, w1 = ftrl_closed_form(z_P, z_w, n_P, n_w, G0, eta0, alpha, beta, gamma, reg)
    np.testing.assert_allclose(P1, P, rtol=1e-12, atol=0)
    np.testing.assert_allclose(w1, w, rtol=1e-12, atol=0)
