"""``spfm_explain_*`` and what ``sparsepoly_amd.explain`` builds on them, on the device.  Needs a
real MI355X: ``pytest -m gpu``.

Values are compared with the NumPy restatement ``restate_contributions(..., wide=True)``
(``tests/test_explain_host.py`` holds it equal to brute-force Shapley values).  The bound comes
from the arithmetic of ``explain_block_kernel`` (``csrc/spfm_explain.hip.h``) and from no device
run.  A computed value is a sum of signed terms ``x_ij p_sj (c_st / t) (-p_sj x_ij)^r m``, ``m`` a
monomial of ``a_{t-1-r}`` (the downdate adds terms that cancel in exact arithmetic, so they are
counted with their magnitudes).  Such a term goes through at most

    N = n_i + 6 M + min(k, 64) + n_blocks ceil(k / 64)

roundings (``n_i`` the row's stored entries, ``M`` the degree):
  * inside ``a_{t-1-r}``: one per factor ``p x``, one per multiplication by it, one per addition of
    the recurrence, of which a row has ``n_i``: ``n_i + 2 (t - 1 - r)``;
  * the downdate: the subtraction that takes ``a_{t-1-r}`` in, then per step the factor ``p x``,
    the product and the subtraction: ``1 + 3 r``; together at most ``n_i + 3 M - 2``;
  * ``c / t``, its product with ``g`` and the ``M - 1`` additions of the sum over ``t``: ``M + 1``;
  * the product with ``p``, the sum over the components of a chunk (``min(k, 64)`` additions) and
    the product with ``x``: ``min(k, 64) + 2``;
  * one addition into the entry per chunk of 64 components and block:
    ``n_blocks ceil(k / 64)`` (the linear term ``w x`` is one rounding and the same additions);
  * ``fit_lower='augment'``: ``c_st`` is the host's sum of products of at most ``M - 1`` dummy
    parameters, ``2 (M - 1)`` roundings.
So ``|device - exact| <= (N + 2) 2^-53 S_hat`` per entry, ``S_hat`` the sum of the magnitudes of
the entry's terms (``majorant`` of ``tests/test_explain_host.py``, computed from magnitudes in
``longdouble``); the 2 covers the second-order terms and the ``longdouble`` reference.  A row sum
adds ``ceil(n_i / 64) + 6`` roundings (lane sums, butterfly).  Each case prints its largest error
as a fraction of its bound before asserting.

Orders are exact.  Where the device order is compared with NumPy's, the NumPy side first asserts,
before the device is touched, that the top K + 1 magnitudes of every row are at least
``CLEAR * max|phi|`` apart; the seeds pass that on the CPU and no case is skipped.
"""

import numpy as np
import pytest
import scipy.sparse as sp
from test_explain_host import COMBOS, majorant, model_output, rows_matrix
from test_ranking_host import abs_model, fm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLEAR = 1e-9
LENGTHS = [0, 1, 2, 63, 64, 65, 130, 700, 5, 0]  # empty first and last row
D = 800
SMALL = [0, 1, 2, 5, 9, 0]


def _roundings(est, Xc):
    """N per stored entry"""
    degree, _, lower = est._obj_pred_args()
    k = est.lams_.shape[0]
    n_i = np.repeat(np.diff(Xc.indptr), np.diff(Xc.indptr))
    return n_i + 6 * degree + min(k, 64) + (2 if lower else 1) * -(-k // 64)


def _reference(est, X, mode):
    """(canonical X, exact values, base, bound per entry), all NumPy"""
    from sparsepoly_amd.explain import restate_contributions

    Xc, want, base = restate_contributions(est, X, mode, wide=True)
    S, _ = majorant(est, X, mode)
    return Xc, want, base, (_roundings(est, Xc) + 2) * U * S


def _check_values(got, want, bound, what):
    assert want.dtype == np.longdouble and got.shape == want.shape
    err = np.abs(got.astype(np.longdouble) - want)
    ok = bound > 0
    frac = float((err[ok] / bound[ok]).max(initial=0.0))
    print("%s: largest error %.3g of its bound" % (what, frac))
    assert (err <= bound).all(), (what, frac)


def _check_estimator(est, X, what):
    for mode, call in (("attribution", est.feature_contributions), ("gradient", est.input_gradient)):
        Xc, want, base, bound = _reference(est, X, mode)
        got = call(X)
        assert sp.isspmatrix_csr(got) and got.dtype == np.float64 and got.shape == Xc.shape
        assert (got.indptr == Xc.indptr).all() and (got.indices == Xc.indices).all()
        _check_values(got.data, want, bound, "%s %s" % (what, mode))


# ---------------------------------------------------------------- 1. values and gradients
def _estimators():
    from sparsepoly_amd import SparseFactorizationMachineClassifier

    cases = [pytest.param((None, dg, fl, lin), id="reg-%d-%s-%d" % (dg, fl, lin))
             for dg, fl, lin in COMBOS]
    for dg, fl in ((3, "explicit"), (5, "augment")):
        cases.append(pytest.param((SparseFactorizationMachineClassifier, dg, fl, True),
                                  id="classifier-%d-%s-1" % (dg, fl)))
    return cases


@pytest.mark.parametrize("spec", _estimators())
def test_values_equal_the_restatement(spec):
    cls, degree, fl, lin = spec
    est = fm(degree, 5, 12, fl, lin, seed=30 + degree, cls=cls)
    _check_estimator(est, rows_matrix(SMALL, 12, seed=degree), "small")


@pytest.mark.parametrize("k,degree,fl", [(k, dg, None) for k in (1, 30, 64, 65, 130)
                                         for dg in (2, 3)]
                         + [(30, 4, None), (30, 5, None), (30, 6, None), (65, 3, "explicit"),
                            (30, 6, "augment")])
def test_shapes_components_and_row_lengths(k, degree, fl):
    """component counts around the chunk of 64, rows around the sweep of 64 entries and far
    beyond it, the two-block model and the coefficient table at length"""
    est = fm(degree, k, D, fl, True, seed=40 + k + degree)
    _check_estimator(est, rows_matrix(LENGTHS, D, seed=k), "k=%d" % k)


def test_dense_and_csc_input_and_base():
    est = fm(3, 30, 40, "augment", True, seed=5)
    X = rows_matrix([0, 3, 40, 17, 0], 40, seed=5)
    Xc, want, base, bound = _reference(est, X, "attribution")
    for form in (X.tocsc(), X.toarray()):
        got, b = est.feature_contributions(form, return_base=True)
        assert (got.indptr == Xc.indptr).all() and (got.indices == Xc.indices).all()
        _check_values(got.data, want, bound, type(form).__name__)
        assert b == float(base)
    assert base != 0  # degree 3, augment, linear: one dummy column with a linear weight


def test_f32_storage_sees_the_same_inputs():
    """precision='f32': x is rounded to float32 first, so both sides see the same inputs; the
    arithmetic is f64 for either storage type and the bound is unchanged"""
    est = fm(3, 30, D, "explicit", True, seed=6)
    est.precision = "f32"
    X = rows_matrix(LENGTHS, D, seed=6, f32=True)
    _check_estimator(est, X, "f32")


# ---------------------------------------------------------------- 2. efficiency
@pytest.mark.parametrize("degree,fl,lin", [(2, None, True), (3, "explicit", True),
                                           (4, "augment", True), (5, "augment", False),
                                           (6, None, False)])
def test_row_sums_plus_base_equal_the_prediction(degree, fl, lin):
    """rowsum + base against the existing predict kernel, within the sum of the two derived
    bounds.  predict: a monomial of a_M passes n_i' + 2 M roundings (n_i' counts the dummy
    columns), then ceil(k / 64) lane additions, the butterfly's 6, one addition per block; the
    linear term one product and n_i' + 1 additions."""
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.explain import _model

    est = fm(degree, 65, D, fl, lin, seed=50 + degree)
    X = rows_matrix(LENGTHS, D, seed=degree)
    Xc, blocks, coef, P, w, lams, lin_, base = _model(est, X)
    S, base_abs = majorant(est, X, "attribution")
    n_i = np.diff(Xc.indptr)
    row = np.repeat(np.arange(Xc.shape[0]), n_i)
    S_row = np.bincount(row, weights=S.astype(np.double), minlength=Xc.shape[0])
    N_row = (n_i + 6 * degree + 64 + len(blocks) * 2) + -(-n_i // 64) + 6 + 1
    bound = (N_row + 2) * U * (S_row + float(base_abs))
    n_dummy = est.P_.shape[2] - D
    N_pred = n_i + n_dummy + 2 * degree + 2 + 6 + len(blocks) + 2
    S_abs = model_output(abs_model(est), np.abs(X.toarray()))
    bound = bound + (N_pred + 2) * U * S_abs
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(P, w, lams)
        vals, rs = eng.explain(Xc, blocks, coef, lin_)
    finally:
        eng.close()
    pred = est.predict(X)
    err = np.abs(rs + base - pred)
    ok = bound > 0
    print("efficiency: largest error %.3g of its bound" % float((err[ok] / bound[ok]).max()))
    assert (err <= bound).all()
    assert rs[0] == 0 and rs[-1] == 0


# ---------------------------------------------------------------- 3. partition independence
def test_one_set_of_bits_under_every_partition():
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.explain import _model

    est = fm(3, 65, D, "explicit", True, seed=7)
    X = rows_matrix(LENGTHS, D, seed=7)
    Xc, blocks, coef, P, w, lams, lin, base = _model(est, X)
    nnz = sum(LENGTHS)
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(P, w, lams)
        got = {}
        # 100: rows 0-3, then one row each (130 and 700 entries exceed the slab), rows 8-9;
        # 1: the empty first row shares the second row's slab, every other row has its own
        for slab, n_slabs in ((0, 1), (100, 6), (1, len(LENGTHS) - 1)):
            eng.explain_set_partition(slab)
            vals, rs = eng.explain(Xc, blocks, coef, lin)
            info = eng.explain_info()
            assert info["slabs"] == n_slabs and info["slab_nnz"] == slab, info
            grad, _ = eng.explain(Xc, blocks, coef, lin, "gradient", rowsum=False)
            idx, val = eng.explain_topk(Xc, blocks, coef, lin, 7)
            assert eng.explain_info()["slabs"] == n_slabs
            got[slab] = (vals, rs, grad, idx, val)
        assert eng.explain_info()["scratch_kib"] > 0
        with pytest.raises(ValueError, match="explain_set_partition"):
            eng.explain_set_partition(-1)
    finally:
        eng.close()
    assert got[0][0].shape == (nnz,) and np.abs(got[0][0]).min() > 0
    for slab in (100, 1):
        for a, b in zip(got[0], got[slab]):
            assert a.tobytes() == b.tobytes(), slab


# ---------------------------------------------------------------- 4. top-K
def _numpy_topk(want, Xc, K):
    """NumPy's stable order of the exact values, (|phi| descending, column ascending), padded;
    asserts first that the top K + 1 magnitudes of every row are CLEAR * max|phi| apart"""
    n = Xc.shape[0]
    cols = np.full((n, K), -1, dtype=np.int32)
    vals = np.zeros((n, K), dtype=np.longdouble)
    pos = np.full((n, K), -1, dtype=np.int64)
    scale = np.abs(want).max()
    for i in range(n):
        b, e = Xc.indptr[i], Xc.indptr[i + 1]
        mag = np.abs(want[b:e])
        order = np.argsort(-mag, kind="stable")  # columns ascend within a canonical row
        top = mag[order][:K + 1]
        if top.size > 1:
            assert np.diff(-top).min() > CLEAR * scale, "top K + 1 magnitudes too close"
        m = min(K, e - b)
        cols[i, :m] = Xc.indices[b:e][order[:m]]
        vals[i, :m] = want[b:e][order[:m]]
        pos[i, :m] = b + order[:m]
    return cols, vals, pos


@pytest.mark.parametrize("K", [1, 5, 64])
def test_top_k_is_numpys_order(K):
    est = fm(3, 30, D, "explicit", True, seed=8)
    X = rows_matrix(LENGTHS, D, seed=8)
    Xc, want, base, bound = _reference(est, X, "attribution")
    cols, vals, pos = _numpy_topk(want, Xc, K)
    got_c, got_v = est.top_contributions(X, K)
    assert got_c.dtype == np.int32 and got_v.dtype == np.float64
    assert got_c.shape == got_v.shape == (len(LENGTHS), K)
    assert (got_c == cols).all()
    filled = pos >= 0
    assert (got_v[~filled] == 0).all() and (got_c[~filled] == -1).all()
    _check_values(got_v[filled], vals[filled], bound[pos[filled]], "top-%d" % K)
    # rows shorter than K are padded: the empty rows entirely
    assert (got_c[0] == -1).all() and (got_c[-1] == -1).all()
    if K > 5:
        assert (got_c[8, :5] >= 0).all() and (got_c[8, 5:] == -1).all()
    # the listed values are the device's own values of those entries
    full = est.feature_contributions(X)
    assert (got_v[filled] == full.data[pos[filled]]).all()


def test_top_k_above_the_cap_is_refused():
    est = fm(2, 3, 10)
    X = rows_matrix([2, 3], 10)
    with pytest.raises(ValueError, match="exceeds the cap"):
        est.top_contributions(X, 65)
    cols, vals = est.top_contributions(X, 64)  # the cap itself is served
    assert cols.shape == (2, 64)


def test_top_k_tie_goes_to_the_lower_column():
    """columns 3 and 9 of P_ and w_ identical, equal x in a row: bit-equal contributions, the
    lower column first"""
    est = fm(3, 5, 12, "explicit", True, seed=9)
    est.P_[:, :, 9] = est.P_[:, :, 3]
    est.w_[9] = est.w_[3]
    X = sp.csr_matrix(np.array([[0, 1.5, 0, 0.75, 0, 0, -2.0, 0, 0, 0.75, 0, 0.5],
                                [0.5, 0, 0, -1.25, 0, 0, 0, 0, 0, -1.25, 0, 0]]))
    full = est.feature_contributions(X).toarray()
    assert (full[:, 3] == full[:, 9]).all() and (full[:, 3] != 0).all()
    cols, vals = est.top_contributions(X, 5)
    for i in range(2):
        c = list(cols[i])
        assert c.index(9) == c.index(3) + 1
        assert vals[i, c.index(3)] == vals[i, c.index(9)] == full[i, 3]
    assert (cols[0] >= 0).all() and list(cols[1, 3:]) == [-1, -1]


# ---------------------------------------------------------------- 5. errors, through the C ABI
def test_errors():
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    est = fm(2, 3, 10)
    X = rows_matrix([2, 0, 3], 10)
    ia, ja, da = _capi.i64(X.indptr), _capi.i32(X.indices), _capi.f64(X.data)
    order, degree = _capi.i32(np.zeros(1)), _capi.i32(np.array([2]))
    coef = np.zeros((1, 3, 7))
    coef[0, :, 2] = 1
    coef = _capi.f64(coef)
    vals, rs = np.full(X.nnz, 7.0), np.full(3, 7.0)
    idx, val = np.full((3, 2), 7, dtype=np.int32), np.full((3, 2), 7.0)
    eng = HipEngine(0, "f64")
    lib, h = eng._lib, eng._h

    def values(n=3, ja=ja, order=order, degree=degree):
        return lib.spfm_explain_csr(h, n, ia[1], ja[1], da[1], 1, order[1], degree[1], coef[1], 1,
                                    0, vals.ctypes.data_as(_capi._dp),
                                    rs.ctypes.data_as(_capi._dp))

    def topk(K):
        return lib.spfm_explain_topk_csr(h, 3, ia[1], ja[1], da[1], 1, order[1], degree[1],
                                         coef[1], 1, K, idx.ctypes.data_as(_capi._ip),
                                         val.ctypes.data_as(_capi._dp))

    def message():
        return lib.spfm_last_error(h).decode()

    try:
        assert values() == _capi.SPFM_ERR_INVALID and "no parameters set" in message()
        assert topk(1) == _capi.SPFM_ERR_INVALID and "no parameters set" in message()
        eng.set_params(est.P_, est.w_, est.lams_)
        assert values(degree=_capi.i32(np.array([7]))) == _capi.SPFM_ERR_UNSUPPORTED
        assert "degree outside 2..6" in message()
        assert values(degree=_capi.i32(np.array([1]))) == _capi.SPFM_ERR_UNSUPPORTED
        assert values(order=_capi.i32(np.array([1]))) == _capi.SPFM_ERR_INVALID
        assert "order_idx outside the parameters" in message()
        bad = X.indices.copy()
        bad[-1] = 10  # = d
        assert values(ja=_capi.i32(bad)) == _capi.SPFM_ERR_INVALID
        assert "column index out of range" in message()
        assert topk(0) == _capi.SPFM_ERR_INVALID and "K must be >= 1" in message()
        assert topk(65) == _capi.SPFM_ERR_UNSUPPORTED and "SPFM_EXPLAIN_MAX_K" in message()
        # nothing was written by any refused call, nor by n = 0
        assert values(n=0) == _capi.SPFM_OK
        assert (vals == 7).all() and (rs == 7).all() and (idx == 7).all() and (val == 7).all()
        assert values() == _capi.SPFM_OK and topk(2) == _capi.SPFM_OK
        assert (vals != 7).all() and rs[1] == 0 and list(idx[1]) == [-1, -1]
        with pytest.raises(ValueError, match="mode must be"):
            eng.explain(X, [(0, 2)], coef[0], True, "shap")
        with pytest.raises(ValueError, match="coef must be"):
            eng.explain(X, [(0, 2)], coef[0][:, :2], True)
        eng.set_params(est.P_, est.w_, est.lams_)  # new parameters: the scratch is gone
        assert eng.explain_info()["scratch_kib"] == 0
    finally:
        eng.close()
