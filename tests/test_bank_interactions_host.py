"""The parts of the bank's consensus interactions that need no device: the
NumPy restatement, the argument checks and host logic of the ``ModelBank`` methods, and the three
C entries' refusal of a NULL handle."""
import ctypes as C

import numpy as np
import pytest


def test_restatement_on_a_worked_case():
    from sparsepoly_amd.interactions import restate_bank_counts

    P0 = np.array([[1.0, 2.0, 0.0, 1.0]])            # W0[0,1] = 2, [0,3] = 1, [1,3] = 2
    P1 = np.array([[1.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0]])  # lams (-1, 1): W1[0,1] = 1
    ref = restate_bank_counts([P0, P1], [np.ones(1), np.array([-1.0, 1.0])], tol=1.0)
    want = np.zeros((4, 4), dtype=np.int64)
    want[0, 1] = want[1, 3] = 1  # |2| > 1 only; the values at 1 are not strictly above
    np.testing.assert_array_equal(ref["count"], want)
    np.testing.assert_array_equal(ref["n_pos"], want)
    assert ref["sum"][0, 1] == 2.0 and ref["sum"][1, 3] == 2.0
    assert ref["histogram"].tolist() == [4, 2, 0] and ref["per_member"].tolist() == [2, 0]
    ref0 = restate_bank_counts([P0, P1], [np.ones(1), np.array([-1.0, 1.0])])
    assert ref0["count"][0, 1] == 2 and ref0["n_pos"][0, 1] == 2 and ref0["sum"][0, 1] == 3.0
    assert ref0["count"][0, 2] == 1 and ref0["n_pos"][0, 2] == 0 and ref0["sum"][0, 2] == -1.0
    with pytest.raises(ValueError):
        restate_bank_counts([P0], [np.ones(1)], tol=-1.0)


@pytest.mark.parametrize("hist, K, want", [([9, 5, 3, 1], 1, 3), ([9, 5, 3, 1], 2, 2),
                                           ([9, 5, 3, 1], 4, 2), ([9, 5, 3, 1], 5, 1),
                                           ([9, 5, 3, 1], 99, 1), ([9, 0, 0, 0], 1, 1),
                                           ([9, 5, 3, 1], 0, 3)])
def test_count_level_of_the_top_k(hist, K, want):
    from sparsepoly_amd.bank import _top_min_count

    assert _top_min_count(np.array(hist), K) == want


def test_order_and_argument_checks():
    from sparsepoly_amd.bank import _check_min_count, _check_tol, _stable_order

    rows, cols = np.array([0, 0, 1, 2]), np.array([1, 2, 2, 3])
    order = _stable_order(rows, cols, np.array([1, 2, 2, 2], dtype=np.int32), None,
                          np.array([9.0, -1.0, 3.0, -3.0]))
    assert order.tolist() == [2, 3, 1, 0]  # count, then |sum|, then (row, col)
    for bad in (0, 4, 1.5):
        with pytest.raises(ValueError, match="min_count"):
            _check_min_count("f()", bad, 3)
    assert _check_min_count("f()", 3, 3) == 3
    for bad in (-1e-300, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            _check_tol("f()", bad)


def test_entries_are_listed_and_refuse_a_null_handle():
    from sparsepoly_amd import _capi

    names = ["spfm_bank_interaction_hist", "spfm_bank_interaction_list",
             "spfm_bank_interaction_counts"]
    assert set(names) <= set(_capi.SYMBOLS)
    L = _capi.load()
    n = C.c_int64()
    assert L.spfm_bank_interaction_hist(None, 0, 4, 0.0, 0, None, None) == _capi.SPFM_ERR_INVALID
    assert L.spfm_bank_interaction_list(None, 0, 4, 0.0, 1, 0, 0, None, None, None, None, None,
                                        C.byref(n)) == _capi.SPFM_ERR_INVALID
    assert L.spfm_bank_interaction_counts(None, 0, 4, 0.0, 0, None, None, None, None,
                                          None) == _capi.SPFM_ERR_INVALID
