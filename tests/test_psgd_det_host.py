"""Deterministic psgd, the parts that need no GPU: the two C entries are
declared and listed, and the estimators' class attribute travels with the clones."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spfm_psgd_set_deterministic", "spfm_psgd_get_deterministic")


@pytest.mark.parametrize("name", NAMES)
def test_entry_is_declared_and_listed(name):
    from sparsepoly_amd import _capi

    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        assert re.search(r"^int %s\(spfm_handle h, " % name, f.read(), re.M)
    assert name in _capi.SYMBOLS


def test_attribute_defaults_to_false_and_survives_the_clone_helper():
    import sparsepoly_amd as sa
    from sparsepoly_amd.model_selection import _clones

    for cls in (sa.SparseFactorizationMachineRegressor, sa.SparseFactorizationMachineClassifier,
                sa.SparseAllSubsetsRegressor, sa.SparseAllSubsetsClassifier):
        assert cls.deterministic is False and "deterministic" not in cls().get_params()
    est = sa.SparseFactorizationMachineRegressor(solver="psgd", regularizer="l1")
    params, make = _clones(est, {"gamma": [0.1, 0.2]})
    assert make(params[0]).deterministic is False
    est.deterministic = True
    assert all(make(p).deterministic is True for p in params)
