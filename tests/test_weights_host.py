"""sparsepoly_amd/weights.py -- validation, class weights and the replication restatement -- and the
declarations of the two row-weight entries.  No device."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from sparsepoly_amd import _capi
from sparsepoly_amd.weights import (check_sample_weight, class_weight_vector, combine_weights,
                                    replicate_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("bad", [
    [1.0, 2.0],                    # wrong length
    [1.0, -0.5, 2.0],              # negative
    [1.0, np.nan, 2.0],
    [1.0, np.inf, 2.0],
    [0.0, 0.0, 0.0],               # all zero
    [[1.0, 1.0, 1.0]],             # not 1-d
])
def test_check_sample_weight_rejects(bad):
    with pytest.raises(ValueError):
        check_sample_weight(bad, 3)


def test_check_sample_weight_accepts_ints_and_lists():
    w = check_sample_weight([2, 0, 1], 3)
    assert w.dtype == np.float64 and w.flags.c_contiguous
    np.testing.assert_array_equal(w, [2.0, 0.0, 1.0])
    w = check_sample_weight(np.array([3, 1, 4], dtype=np.int32)[::1], 3)
    np.testing.assert_array_equal(w, [3.0, 1.0, 4.0])
    strided = np.arange(6, dtype=np.float64)[::2]       # not contiguous on the way in
    assert check_sample_weight(strided, 3).flags.c_contiguous


def test_class_weight_vector_balanced():
    y = np.array([3, 3, 7, 3, 9, 7, 3, 3])
    counts = np.bincount(np.unique(y, return_inverse=True)[1])   # (5, 2, 1) for 3, 7, 9
    per_class = y.size / (3 * counts.astype(float))
    expected = per_class[np.unique(y, return_inverse=True)[1]]
    np.testing.assert_array_equal(class_weight_vector("balanced", y), expected)
    # sklearn's property: the weights of each class sum to n / n_classes
    v = class_weight_vector("balanced", y)
    for c in (3, 7, 9):
        np.testing.assert_allclose(v[y == c].sum(), y.size / 3.0, rtol=1e-15)


def test_class_weight_vector_dict_none_and_errors():
    y = np.array([-1, 1, 1, -1, 1])
    np.testing.assert_array_equal(class_weight_vector(None, y), np.ones(5))
    np.testing.assert_array_equal(class_weight_vector({1: 2.5}, y), [1, 2.5, 2.5, 1, 2.5])
    np.testing.assert_array_equal(class_weight_vector({1: 2, -1: 0}, y), [0, 2, 2, 0, 2])
    ys = np.array(["a", "b", "a"])
    np.testing.assert_array_equal(class_weight_vector({"b": 4}, ys), [1, 4, 1])
    with pytest.raises(ValueError):
        class_weight_vector({5: 2.0}, y)             # an unknown label
    with pytest.raises(ValueError):
        class_weight_vector({1: -1.0}, y)
    with pytest.raises(ValueError):
        class_weight_vector("balance", y)
    with pytest.raises(ValueError):
        class_weight_vector(3.0, y)


def test_combine_weights():
    y = np.array([-1, 1, 1, -1])
    assert combine_weights(None, None, y, 4) is None
    np.testing.assert_array_equal(combine_weights([1, 2, 3, 4], None, y, 4), [1, 2, 3, 4])
    np.testing.assert_array_equal(combine_weights([1, 2, 3, 4], {1: 10}, y, 4), [1, 20, 30, 4])
    np.testing.assert_array_equal(combine_weights(None, "balanced", y, 4), np.ones(4))
    with pytest.raises(ValueError):
        combine_weights([0, 1, 1, 0], {1: 0}, y, 4)  # the product is all zero


def test_replicate_rows():
    rng = np.random.RandomState(0)
    X = sp.random(5, 7, density=0.5, random_state=rng, format="csr")
    y = np.arange(5, dtype=float) * 1.5
    w = (2, 0, 1, 3, 1)
    Xr, yr = replicate_rows(X, y, w)
    rows = [0, 0, 2, 3, 3, 3, 4]                      # row 1 is dropped, order is kept
    assert sp.isspmatrix_csr(Xr) and Xr.shape == (7, 7) and Xr.has_sorted_indices
    np.testing.assert_array_equal(Xr.toarray(), X.toarray()[rows])
    np.testing.assert_array_equal(yr, y[rows])
    Xd, yd = replicate_rows(X.toarray(), y, w)        # dense in, dense out
    np.testing.assert_array_equal(Xd, X.toarray()[rows])
    np.testing.assert_array_equal(yd, y[rows])
    Xc, _ = replicate_rows(X.tocsc(), y, w)
    np.testing.assert_array_equal(Xc.toarray(), X.toarray()[rows])
    with pytest.raises(ValueError):
        replicate_rows(X, y, (1, 1, 0.5, 1, 1))      # not integer
    with pytest.raises(ValueError):
        replicate_rows(X, y, (1, 1, 1))


def test_replication_is_the_weighted_sum():
    """the property the device tests pin, on the two sums themselves"""
    rng = np.random.RandomState(3)
    x, dl = rng.randn(9), rng.randn(9)
    w = np.array([2, 0, 1, 3, 1, 0, 0, 2, 1])
    Xr, dr = replicate_rows(x[:, None], dl, w)
    np.testing.assert_allclose(np.sum(w * dl * x), np.sum(dr * Xr[:, 0]), rtol=1e-13)
    np.testing.assert_allclose(np.sum(w * x * x), np.sum(Xr[:, 0] ** 2), rtol=1e-13)


def test_prototypes_declared():
    with open(os.path.join(ROOT, "include", "spfm.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert ("int spfm_set_sample_weight(spfm_handle h, const double* weights, int64_t n);"
            in header)
    assert ("int spfm_get_sample_weight(spfm_handle h, int* set_out, double* sum_out);"
            in header)
    assert "spfm_set_sample_weight" in _capi.SYMBOLS
    assert "spfm_get_sample_weight" in _capi.SYMBOLS
    with open(os.path.join(ROOT, "sparsepoly_amd", "_capi.py")) as f:
        src = f.read()
    assert "L.spfm_set_sample_weight.argtypes" in src
    assert "L.spfm_get_sample_weight.argtypes" in src


def test_estimators_take_the_keyword_and_keep_their_parameters():
    import inspect

    from sparsepoly_amd import (SparseAllSubsetsClassifier,
                                SparseAllSubsetsRegressor, SparseFactorizationMachineClassifier,
                                SparseFactorizationMachineRegressor)
    from sparsepoly_amd.concurrent import fit_concurrently
    from sparsepoly_amd.multiclass import OneVsRestClassifier

    for cls in (SparseFactorizationMachineRegressor, SparseFactorizationMachineClassifier,
                SparseAllSubsetsRegressor, SparseAllSubsetsClassifier, OneVsRestClassifier):
        sig = inspect.signature(cls.fit)
        assert sig.parameters["sample_weight"].default is None
    for cls in (SparseFactorizationMachineClassifier, SparseAllSubsetsClassifier):
        assert cls.class_weight is None
        assert "class_weight" not in cls().get_params()
    assert OneVsRestClassifier.class_weight is None
    p = inspect.signature(fit_concurrently).parameters["sample_weights"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
