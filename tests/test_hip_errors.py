"""Refusals and edge shapes of the host engine's shared plumbing (typed copies, CSR staging,
target upload, storage-type dispatch, entry guard).

* Every refused call of tools/record_errors.py answers with the return code and the message the
  parent commit gave (profiles/errors_parent_438713e297d8.json), for both storage types.
* The same for the psgd unit's own table (profiles/errors_psgd_parent_06084fb635e5.json, recorded
  on the commit before the unit's shared pieces were folded into one copy each).
* Shapes at which a count is 0 or a buffer is shared behave as before: they pin behaviour, each
  of them passes on the parent commit too.

Needs a real MI355X."""
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_errors as rec  # noqa: E402

pytestmark = pytest.mark.gpu

PARENT = os.path.join(ROOT, "profiles", "errors_parent_438713e297d8.json")
PSGD_PARENT = os.path.join(ROOT, "profiles", "errors_psgd_parent_06084fb635e5.json")
DTYPES = ("f32", "f64")
N, D, K = rec.N, rec.D, rec.K


def _engine(dtype):
    from sparsepoly_amd.engine import HipEngine

    return HipEngine(0, dtype)


def _X():
    return sp.csr_matrix((rec.DATA, rec.INDICES, rec.INDPTR), shape=(N, D))


def _model(dtype, X=None, y=None, configure=True):
    eng = _engine(dtype)
    eng.set_data(_X() if X is None else X, rec.Y if y is None else y)
    eng.set_params(rec.P, rec.W, rec.LAMS)
    if configure:
        eng.configure("pcd", "squared", "l1", 2)
    return eng


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_answer_as_on_the_parent(dtype):
    with open(PARENT) as f:
        want = json.load(f)["cases"][dtype]
    assert set(want) == {name for name, _, _ in rec.CASES}
    assert sum(rc != 0 for rc, _ in want.values()) == len(want)  # every case is a refusal
    lib = rec._capi.load()
    got = {name: rec.run_case(lib, dtype, state, call) for name, state, call in rec.CASES}
    diff = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    assert not diff, diff


@pytest.mark.parametrize("dtype", DTYPES)
def test_psgd_refusals_answer_as_on_the_parent(dtype):
    with open(PSGD_PARENT) as f:
        want = json.load(f)["cases"][dtype]
    assert set(want) == {name for name, _, _ in rec.PSGD_CASES}
    assert sum(rc != 0 for rc, _ in want.values()) == len(want)  # every case is a refusal
    lib = rec._capi.load()
    got = {name: rec.run_psgd_case(lib, dtype, state, call)
           for name, state, call in rec.PSGD_CASES}
    diff = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    assert not diff, diff


# --------------------------------------------------------------- edge shapes
@pytest.mark.parametrize("fmt", ("csr", "csc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_training_matrix_without_entries(dtype, fmt):
    X = sp.csr_matrix((N, D)) if fmt == "csr" else sp.csc_matrix((N, D))
    eng = _model(dtype, X=X)
    eng.init_pred(2, True, False)
    assert np.array_equal(eng.get_y_pred(), np.zeros(N))
    y = rec.Y.astype(np.float32).astype(np.float64) if dtype == "f32" else rec.Y
    # 0.5 * sum y^2 in double from the stored targets, N positive terms summed in another
    # order: N * 2^-53 relative at the most
    assert eng.loss_sum() == pytest.approx(0.5 * float(np.sum(y * y)), rel=1e-14)
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_predict_on_no_rows_and_on_empty_rows(dtype):
    eng = _model(dtype, configure=False)
    out = eng.predict(sp.csr_matrix((0, D)), 2, True, False)
    assert out.shape == (0,)
    # spfm_predict_csr leaves `out` alone for 0 rows
    keep = np.full(3, 7.0)
    rc = eng._lib.spfm_predict_csr(eng._h, 0, rec.ptr(rec.i64(0)), None, None, 2, 1, 0,
                                   rec.ptr(keep))
    assert rc == 0 and np.array_equal(keep, np.full(3, 7.0))
    out = eng.predict(sp.csr_matrix((4, D)), 2, True, True)
    assert np.array_equal(out, np.zeros(4))
    eng.close()


@pytest.mark.parametrize("with_y", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_held_out_set_without_entries(dtype, with_y):
    eng = _model(dtype)
    y = np.array([0.5, -2.0, 3.0])
    eng.set_eval_data(sp.csr_matrix((3, D)), y if with_y else None)
    loss, pred = eng.eval_loss(2, True, False, return_pred=True)
    assert np.array_equal(pred, np.zeros(3))
    if with_y:
        assert loss == pytest.approx(0.5 * float(np.sum(y * y)), rel=1e-14)
    else:
        assert loss is None
    # ... and no rows at all
    eng.set_eval_data(sp.csr_matrix((0, D)), np.zeros(0) if with_y else None)
    loss, pred = eng.eval_loss(2, True, False, return_pred=True)
    assert pred.shape == (0,) and (loss == 0.0 if with_y else loss is None)
    eng.close()


def _gram(eng, kind, degree, X, B=None, Pm=None, lams=None, budget=0):
    n1, d = X.shape
    ip, ix, dat = rec.ptr(X.indptr.astype(np.int64)), rec.ptr(X.indices.astype(np.int32)), \
        rec.ptr(X.data.astype(np.float64))
    n2 = (B if B is not None else Pm).shape[0]
    out = np.full(n1 if lams is not None else n1 * n2, np.nan)
    lp = rec.ptr(lams) if lams is not None else None
    if B is not None:
        rc = eng._lib.spfm_gram_csr_dense(eng._h, kind, degree, n1, d, ip, ix, dat, n2,
                                          rec.ptr(B), lp, 0, budget, rec.ptr(out))
    else:
        rc = eng._lib.spfm_gram_csr_csr(eng._h, kind, degree, n1, d, ip, ix, dat, n2,
                                        rec.ptr(Pm.indptr.astype(np.int64)),
                                        rec.ptr(Pm.indices.astype(np.int32)),
                                        rec.ptr(Pm.data.astype(np.float64)), lp, budget,
                                        rec.ptr(out))
    assert rc == 0, eng._lib.spfm_last_error(eng._h)
    return out


@pytest.mark.parametrize("lams", (False, True))
@pytest.mark.parametrize("form", ("dense", "csr"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_gram_one_row_per_block_is_bit_equal(dtype, form, lams):
    """A budget of one byte: one row of X per block, one 64-column chunk per tile (130 columns:
    three tiles, the last of two columns); an empty row of X goes through a block of its own."""
    rng = np.random.RandomState(3)
    X = sp.random(5, 7, density=0.5, random_state=rng, format="csr")
    X = sp.vstack([X[:2], sp.csr_matrix((1, 7)), X[2:4]]).tocsr()  # 5 x 7, row 2 empty
    X.sort_indices()
    B = rng.randn(130, 7)
    lm = np.where(rng.rand(130) < 0.5, 1.0, -1.0) if lams else None
    kw = dict(B=B) if form == "dense" else dict(Pm=sp.csr_matrix(B * (rng.rand(130, 7) < 0.6)))
    eng = _engine(dtype)
    for kind, degree in ((0, 3), (1, 2), (2, 0)):
        want = _gram(eng, kind, degree, X, lams=lm, **kw)
        got = _gram(eng, kind, degree, X, lams=lm, budget=1, **kw)
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), (kind, degree)
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_follower_upload_leaves_the_leader_alone(dtype):
    """spfm_share_data, then set_data_csr on the follower: the follower's buffers detach from the
    shared image before anything is written into them."""
    rng = np.random.RandomState(5)
    X = sp.random(40, 12, density=0.3, random_state=rng, format="csr")
    X.sort_indices()
    y = rng.randn(40)
    P, w, lams = rng.randn(1, K, 12) * 0.1, rng.randn(12) * 0.1, np.array([1.0, -1.0])
    X2 = sp.random(40, 12, density=0.4, random_state=rng, format="csr")
    X2.sort_indices()

    def fit(eng):
        eng.set_params(P, w, lams)
        eng.configure("pcd", "squared", "l1", 2)
        eng.set_schedule("colored", np.arange(12, dtype=np.int32))
        eng.init_pred(2, True, False)
        viol = eng.pcd_epoch(0, 2, 0.1, 0.01, 1.0, np.arange(K, dtype=np.int32))
        return eng.get_y_pred(), viol

    solo = _engine(dtype)
    solo.set_data(X, y)
    want = fit(solo)
    solo.close()

    leader, follower = _engine(dtype), _engine(dtype)
    leader.set_data(X, y)
    follower.share_data(leader, -y)
    follower.set_data(X2, 2.0 * y)  # its own image from here on
    got = fit(leader)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    # the follower trains on what it uploaded
    f2 = _engine(dtype)
    f2.set_data(X2, 2.0 * y)
    want2, got2 = fit(f2), fit(follower)
    assert np.array_equal(got2[0], want2[0]) and got2[1] == want2[1]
    for e in (leader, follower, f2):
        e.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_interaction_values_of_no_pairs(dtype):
    eng = _model(dtype)
    vals = eng.interaction_values(0, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert vals.shape == (0,)
    keep = np.full(2, 7.0)
    rc = eng._lib.spfm_interaction_values(eng._h, 0, 0, None, None, rec.ptr(keep))
    assert rc == 0 and np.array_equal(keep, np.full(2, 7.0))
    eng.close()
