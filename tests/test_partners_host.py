"""Host side of the per-feature interaction views (``spfm_interaction_degrees`` / ``_partners``):
the C ABI bookkeeping, the Python argument errors, and the NumPy restatements
``restate_partners`` / ``restate_degrees`` on hand-computed 4-feature blocks.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("spfm_interaction_degrees", "spfm_interaction_partners")


def test_header_capi_and_library_agree():
    import ctypes as C

    from sparsepoly_amd import _capi

    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(spfm_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    for macro, value in (("SPFM_PARTNERS_ABS", 0), ("SPFM_PARTNERS_POS", 1),
                         ("SPFM_PARTNERS_NEG", 2), ("SPFM_INTERACTION_MAX_K", 128)):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, header)
        assert m and int(m.group(1)) == value, macro
    assert _capi.INTERACTION_MAX_K == 128
    assert _capi.PARTNERS_BY == {"abs": 0, "positive": 1, "negative": 2}
    lib = _capi.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p
    assert len(lib.spfm_interaction_degrees.argtypes) == 8
    assert len(lib.spfm_interaction_partners.argtypes) == 13


def _fake(d=6, **kw):
    """An estimator that holds a block and must not open a device session"""
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    est = SparseFactorizationMachineRegressor(degree=2, n_components=2, fit_linear=False, **kw)
    est.P_ = np.ones((1, 2, d))
    est.lams_ = np.ones(2)
    est.w_ = np.zeros(d)

    def no_engine():
        raise AssertionError("a handle was asked for")

    est._new_engine = no_engine
    return est


@pytest.mark.parametrize("kwargs,match", [
    (dict(K=0), "K must be"),
    (dict(K=129), "K must be"),
    (dict(K=2.5), "K must be"),
    (dict(K=3, features=[0, 6]), "out of range"),
    (dict(K=3, features=[-1]), "out of range"),
    (dict(K=3, features=[[0, 1]]), "1-d"),
    (dict(K=3, by="largest"), "by must be"),
    (dict(K=3, among=(3, 3)), "empty"),
    (dict(K=3, among=(4, 2)), "empty"),
    (dict(K=3, among=(0, 7)), "outside"),
    (dict(K=3, among=(-1, 3)), "outside"),
    (dict(K=3, among=(1, 2, 3)), "pair"),
])
def test_argument_errors_before_a_handle_exists(kwargs, match):
    from sparsepoly_amd.interactions import partner_graph

    est = _fake()
    with pytest.raises(ValueError, match=match):
        est.top_partners(**kwargs)
    with pytest.raises(ValueError, match=match):
        partner_graph(est, **kwargs)


def test_other_errors_before_a_handle_exists():
    from sklearn.utils.validation import NotFittedError

    from sparsepoly_amd import SparseFactorizationMachineRegressor

    with pytest.raises(ValueError, match="tol must be >= 0"):
        _fake().interaction_degrees(tol=-1.0)
    est = SparseFactorizationMachineRegressor(degree=3, n_components=2, fit_lower=None)
    with pytest.raises(NotFittedError):
        est.top_partners(3)
    est.P_ = np.ones((1, 2, 6))
    for call in (lambda: est.top_partners(3), lambda: est.interaction_degrees()):
        with pytest.raises(ValueError, match="no degree-2 block"):
            call()
    # fit_lower='augment' without a linear term: one dummy column, and the view ends before it
    aug = _fake(d=7, fit_lower="augment")
    with pytest.raises(ValueError, match=r"out of range \[0, 6\)"):
        aug.top_partners(2, features=[6])
    with pytest.raises(AssertionError, match="handle"):  # valid arguments do reach the engine
        aug.top_partners(2, features=[6], include_augmented=True)


# four features, k = 2, lams = (+1, -1):
#   P = [[1, 2, 0, -1],       W = P^T diag(lams) P =  [[ .,  2,  0, -1],
#        [0, 0, 3,  2]]                                [ 2,  .,  0, -2],
#                                                      [ 0,  0,  ., -6],
#                                                      [-1, -2, -6,  .]]
P4 = np.array([[1.0, 2.0, 0.0, -1.0], [0.0, 0.0, 3.0, 2.0]])
L4 = np.array([1.0, -1.0])
W4 = np.array([[1.0, 2.0, 0.0, -1.0], [2.0, 4.0, 0.0, -2.0], [0.0, 0.0, -9.0, -6.0],
               [-1.0, -2.0, -6.0, -3.0]])


def test_restate_partners_by_hand():
    from sparsepoly_amd.interactions import _dense_w, restate_partners

    np.testing.assert_array_equal(_dense_w(P4, L4), W4)
    ids, vals, counts = restate_partners(P4, L4, 2)
    # row 1: |2| and |-2| tie, id 0 first
    np.testing.assert_array_equal(ids, [[1, 3], [0, 3], [3, -1], [2, 1]])
    np.testing.assert_array_equal(vals, [[2.0, -1.0], [2.0, -2.0], [-6.0, 0.0], [-6.0, -2.0]])
    np.testing.assert_array_equal(counts, [2, 2, 1, 2])
    assert ids.dtype == np.int32 and ids.shape == (4, 2)
    ids, vals, counts = restate_partners(P4, L4, 3, by="positive")
    np.testing.assert_array_equal(ids, [[1, -1, -1], [0, -1, -1], [-1, -1, -1], [-1, -1, -1]])
    np.testing.assert_array_equal(vals, [[2.0, 0, 0], [2.0, 0, 0], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(counts, [1, 1, 0, 0])
    ids, vals, counts = restate_partners(P4, L4, 2, by="negative")
    np.testing.assert_array_equal(ids, [[3, -1], [3, -1], [3, -1], [2, 1]])
    np.testing.assert_array_equal(vals, [[-1.0, 0], [-2.0, 0], [-6.0, 0], [-6.0, -2.0]])
    np.testing.assert_array_equal(counts, [1, 1, 1, 2])
    # among, repeated features, the diagonal (|W4[3, 3]| = 3 would be second in row 3) left out
    ids, vals, counts = restate_partners(P4, L4, 3, features=[3, 1, 3], among=(1, 4))
    np.testing.assert_array_equal(ids, [[2, 1, -1], [3, -1, -1], [2, 1, -1]])
    np.testing.assert_array_equal(vals, [[-6.0, -2.0, 0], [-2.0, 0, 0], [-6.0, -2.0, 0]])
    np.testing.assert_array_equal(counts, [2, 1, 2])
    # K = 1 with a tie in magnitude: the smaller id
    ids, _, _ = restate_partners(P4, L4, 1, features=[1])
    assert ids.tolist() == [[0]]
    # a dense W can be given directly
    a = restate_partners(None, None, 2, W=W4)
    b = restate_partners(P4, L4, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_restate_degrees_by_hand():
    from sparsepoly_amd.interactions import restate_degrees

    r = restate_degrees(P4, L4)
    np.testing.assert_array_equal(r["degree"], [2, 2, 1, 3])
    np.testing.assert_array_equal(r["sum_abs"], [3.0, 4.0, 6.0, 9.0])
    np.testing.assert_array_equal(r["max_abs"], [2.0, 2.0, 6.0, 6.0])
    np.testing.assert_array_equal(r["strongest"], [1, 0, 3, 2])  # feature 1: 0 and 3 tie, 0 wins
    assert r["degree"].dtype == np.int64 and r["strongest"].dtype == np.int32
    r = restate_degrees(P4, L4, tol=1.5)
    np.testing.assert_array_equal(r["degree"], [1, 2, 1, 2])
    r = restate_degrees(P4, L4, tol=2.0)  # strict
    np.testing.assert_array_equal(r["degree"], [0, 0, 1, 1])
    # an inactive feature: empty answers, and it is nobody's partner
    P = np.array([[1.0, 0.0, 2.0]])
    r = restate_degrees(P, np.ones(1))
    np.testing.assert_array_equal(r["degree"], [1, 0, 1])
    np.testing.assert_array_equal(r["strongest"], [2, -1, 0])
    np.testing.assert_array_equal(r["sum_abs"], [2.0, 0.0, 2.0])
    with pytest.raises(ValueError, match="tol"):
        restate_degrees(P4, L4, tol=-1.0)
