"""Third-order interaction weights: what can be checked without a device.  The header and the
ctypes binding agree, the estimators pick the right block, ``support_recovery3`` does the
notebook's arithmetic on triples, and without a GPU the methods raise as the pair methods do.
The device side is ``tests/test_hip_interactions3.py``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from sklearn.utils.validation import NotFittedError

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ("spfm_interaction3_stats", "spfm_interaction3_topk", "spfm_interaction3_list",
           "spfm_interaction3_values")
CTYPES = {"spfm_handle": C.c_void_p, "int": C.c_int, "double": C.c_double, "int64_t": C.c_int64,
          "int64_t*": C.POINTER(C.c_int64), "int32_t*": C.POINTER(C.c_int32),
          "double*": C.POINTER(C.c_double)}


def _declared(name):
    """argument types of ``name`` as include/spfm.h declares them"""
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    m = re.search(r"\bint %s\(([^)]*)\);" % name, header)
    assert m, name
    types = []
    for arg in m.group(1).split(","):
        arg = arg.replace("const ", "").strip()
        t = arg.rsplit(" ", 1)[0].strip()
        types.append(t.replace(" *", "*"))
    return types


def test_header_declares_the_entries_and_capi_binds_them():
    from sparsepoly_amd import _capi

    assert _declared("spfm_interaction3_stats") == [
        "spfm_handle", "int", "double", "int64_t*", "double*"]
    assert _declared("spfm_interaction3_topk") == [
        "spfm_handle", "int", "int64_t", "int32_t*", "int32_t*", "int32_t*", "double*", "int64_t*"]
    assert _declared("spfm_interaction3_list") == [
        "spfm_handle", "int", "double", "int64_t", "int32_t*", "int32_t*", "int32_t*", "double*",
        "int64_t*"]
    assert _declared("spfm_interaction3_values") == [
        "spfm_handle", "int", "int64_t", "int32_t*", "int32_t*", "int32_t*", "double*"]
    lib = _capi.load()
    for name in ENTRIES:
        assert name in _capi.SYMBOLS
        f = getattr(lib, name)
        assert f.restype is C.c_int
        assert list(f.argtypes) == [CTYPES[t] for t in _declared(name)], name
    header = open(os.path.join(ROOT, "include", "spfm.h")).read()
    m = re.search(r"#define SPFM_INTERACTION3_MAX_ACTIVE \(1 << (\d+)\)", header)
    assert m and _capi.INTERACTION3_MAX_ACTIVE == 1 << int(m.group(1)) == 1 << 15


def _fm(**kw):
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    est = SparseFactorizationMachineRegressor(**kw)
    est.P_ = np.zeros((1, 2, 5))  # as after a fit; the block is chosen before any device call
    est.lams_ = np.ones(2)
    return est


def test_block_spec():
    from sparsepoly_amd import SparseAllSubsetsRegressor

    def spec(**kw):
        return _fm(**kw)._interaction3_block_spec("x")

    assert spec(degree=3) == (0, 0)
    assert spec(degree=3, fit_lower=None) == (0, 0)
    assert spec(degree=3, fit_lower="explicit") == (0, 0)
    assert spec(degree=4, fit_lower="explicit") == (1, 0)
    assert spec(degree=5, fit_lower="explicit") == (2, 0)
    # augment: degree - 1 dummy columns, one less when the linear term has its own weights
    assert spec(degree=3, fit_lower="augment", fit_linear=False) == (0, 2)
    assert spec(degree=3, fit_lower="augment", fit_linear=True) == (0, 1)
    est = SparseAllSubsetsRegressor()
    est.P_ = np.zeros((1, 1))
    assert est._interaction3_block_spec("x") == (0, 0)
    # the pair rule is untouched
    assert _fm(degree=3, fit_lower="explicit")._interaction_block_spec("x") == (1, 0)


@pytest.mark.parametrize("kw", [dict(degree=2), dict(degree=2, fit_lower="explicit"),
                                dict(degree=4, fit_lower=None), dict(degree=4, fit_lower="augment"),
                                dict(degree=5, fit_lower="augment")])
def test_no_degree3_block(kw):
    est = _fm(**kw)
    for call in (lambda: est.triple_stats(), lambda: est.top_triples(5), lambda: est.triples(),
                 lambda: est.triple_values([0], [1], [2])):
        with pytest.raises(ValueError, match="no degree-3 block"):
            call()
    with pytest.raises(ValueError, match="degree=%d" % kw["degree"]):
        est.triple_stats()


@pytest.mark.parametrize("idx", range(4))
def test_not_fitted(idx):
    from sparsepoly_amd import (SparseAllSubsetsClassifier, SparseAllSubsetsRegressor,
                                SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)

    est = (SparseFactorizationMachineRegressor, SparseFactorizationMachineClassifier,
           SparseAllSubsetsRegressor, SparseAllSubsetsClassifier)[idx]()
    for call in (lambda: est.triple_stats(), lambda: est.top_triples(5), lambda: est.triples(),
                 lambda: est.triple_values([0], [1], [2])):
        with pytest.raises(NotFittedError):
            call()


class _Stub(object):
    """An estimator whose device calls are answered from a dict of triples; counts its calls."""

    def __init__(self, triples):
        self.T = {tuple(sorted(t)): v for t, v in triples.items()}
        self.calls = []

    def triple_stats(self, tol=0.0, include_augmented=False):
        self.calls.append(("stats", tol))
        return dict(nnz=sum(1 for v in self.T.values() if abs(v) > tol))

    def triple_values(self, i, j, l, include_augmented=False):
        self.calls.append(("values", len(i)))
        return np.array([self.T.get(tuple(sorted(t)), 0.0) for t in zip(i, j, l)], dtype=float)


def test_support_recovery3_arithmetic():
    from sparsepoly_amd.interactions import support_recovery3

    # two of three true triples found (one given in another id order, one twice), one false triple
    est = _Stub({(0, 1, 2): 0.3, (1, 3, 4): -0.2, (2, 3, 5): 0.1})
    true = np.array([(0, 1, 2), (4, 1, 3), (0, 4, 5), (2, 1, 0)])
    r = support_recovery3(est, (true[:, 0], true[:, 1], true[:, 2]))
    assert (r["tp"], r["fp"], r["fn"], r["nnz"]) == (2, 1, 1, 3)
    assert r["fscore"] == pytest.approx(2 * (2 / 3) * (2 / 3) / (4 / 3)) and r["pssr"] is False
    assert est.calls == [("stats", 0.0), ("values", 3)]  # one call each, repeats folded
    # exact recovery
    est = _Stub({(0, 1, 2): 1.0})
    r = support_recovery3(est, ([2], [0], [1]))
    assert r == dict(fscore=1.0, pssr=True, nnz=1, tp=1, fp=0, fn=0)
    # nothing selected: precision 0, F-score 0; empty true support: recall 0
    r = support_recovery3(_Stub({}), ([0], [1], [2]))
    assert r == dict(fscore=0.0, pssr=False, nnz=0, tp=0, fp=0, fn=1)
    r = support_recovery3(_Stub({(0, 1, 2): 1.0}), (np.zeros(0, int),) * 3)
    assert r == dict(fscore=0.0, pssr=False, nnz=1, tp=0, fp=1, fn=0)
    with pytest.raises(ValueError, match="must differ"):
        support_recovery3(_Stub({}), ([0], [0], [2]))
    with pytest.raises(ValueError, match="one length"):
        support_recovery3(_Stub({}), ([0], [1, 2], [2]))


def test_without_a_gpu_the_methods_raise_as_the_pair_methods_do():
    """Whatever a pair method does on this machine (an error without a device, a result with
    one), the triple method of the same estimator does too: there is no CPU path."""
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    rng = np.random.RandomState(0)
    est = SparseFactorizationMachineRegressor(degree=3, fit_lower="explicit", n_components=2)
    est.P_ = rng.randn(2, 2, 6)
    est.lams_ = np.ones(2)
    est.w_ = np.zeros(6)
    try:
        est.interaction_stats()
        pair_error = None
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        pair_error = type(e)
    calls = (lambda: est.triple_stats(), lambda: est.top_triples(3), lambda: est.triples(),
             lambda: est.triple_values([0], [1], [2]))
    if pair_error is None:
        assert est.triple_stats()["nnz"] == 20 and len(est.top_triples(3)[3]) == 3
        assert len(est.triples()[0]) == 20 and est.triple_values([0], [1], [2]).shape == (1,)
    else:
        for call in calls:
            with pytest.raises(pair_error):
                call()
