"""``spfm_interaction3_*`` and the estimators' ``triple_*`` methods on the device.  Needs a real
MI355X: ``pytest -m gpu``.

Reference: ``numpy.einsum('s,sa,sj,sl->ajl', lams, P, P, P)`` in float64 on the host, restricted
to ``a < j < l`` (computed once per block and shared).  Bounds, from the arithmetic alone:

* per value ``|got - ref| <= (k + 3) 2^-52 sum_s |p_sa p_sj p_sl|``: the worst case of a k-term
  sum of triple products in any order (each product two roundings, the sum ``k - 1``), doubled
  because the reference carries the same error;
* ``sum_sq`` / ``sum_abs``: relative to the reference's ``sum T^2`` / ``sum |T|`` at most
  ``N_triples 2^-52``, the worst case of any summation order; ``max_abs`` is one value;
* counts, ids and orders are exact.  Where a device run could legitimately differ (an entry at
  the threshold, two magnitudes of the top K + 1 closer than their errors) the case asserts on
  the NumPy side, before the device is touched, that this is not so.
"""
import ctypes as C
import functools
import pickle

import numpy as np
import pytest
from test_hip_interactions import _engine, _quiet
from test_hip_objective import LIVE, _Live, _problem

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CLEAR = 1e-9


# ------------------------------------------------------------------ reference
def _reference(P, lams):
    """dict: ids ``i, j, l`` (sorted by (i, j, l)), ``vals``, ``bound`` = sum_s |terms| of every
    triple a < j < l of the active features, ``active``"""
    k, d = P.shape
    act = np.flatnonzero((P != 0).any(axis=0))
    Pa = np.ascontiguousarray(P[:, act], dtype=np.float64)
    T = np.einsum("s,sa,sj,sl->ajl", np.asarray(lams, dtype=np.float64), Pa, Pa, Pa,
                  optimize=True)
    Q = np.abs(Pa)
    B = np.einsum("sa,sjl->ajl", Q, Q[:, :, None] * Q[:, None, :], optimize=True)
    n = np.arange(len(act))
    mask = (n[:, None, None] < n[None, :, None]) & (n[None, :, None] < n[None, None, :])
    a, j, l = np.nonzero(mask)
    return dict(i=act[a].astype(np.int32), j=act[j].astype(np.int32), l=act[l].astype(np.int32),
                vals=T[mask], bound=B[mask], active=len(act), k=k)


def _select(ref, tol=0.0):
    """the triples with |T| > tol, in list order"""
    keep = np.abs(ref["vals"]) > tol
    return {key: (v[keep] if isinstance(v, np.ndarray) else v) for key, v in ref.items()}


def _top(ref, K):
    """indices (into a selection) of the K largest |T| != 0 by (|T| desc, i, j, l)"""
    nz = np.flatnonzero(ref["vals"] != 0)
    o = np.lexsort((ref["l"][nz], ref["j"][nz], ref["i"][nz], -np.abs(ref["vals"][nz])))
    return nz[o[:K]]


def _preconditions(ref, K, tol=0.0):
    """no entry within its error of 0 or of tol, the top K + 1 magnitudes apart"""
    k, v, b = ref["k"], np.abs(ref["vals"]), ref["bound"]
    err = (k + 3) * EPS * b
    live = b > 0
    assert not v[~live].any()
    big = v.max(initial=0.0)
    assert (v[live] > 4 * err[live]).all(), "an entry within its error of zero"
    assert (np.abs(v[live] - tol) > 4 * err[live] + CLEAR * big * (tol > 0)).all(), "entry at tol"
    mags = v[_top(ref, K + 1)]
    if len(mags) > 1:
        assert np.diff(-mags).min() > CLEAR * big, "top K + 1 magnitudes too close"


def _check_triples(got, ref, idx, what):
    i, j, l, vals = got
    assert i.dtype == np.int32 and j.dtype == np.int32 and l.dtype == np.int32
    np.testing.assert_array_equal(i, ref["i"][idx], err_msg=str(what))
    np.testing.assert_array_equal(j, ref["j"][idx], err_msg=str(what))
    np.testing.assert_array_equal(l, ref["l"][idx], err_msg=str(what))
    err = np.abs(vals - ref["vals"][idx])
    lim = (ref["k"] + 3) * EPS * ref["bound"][idx]
    print(what, "worst value error as a fraction of its bound: %.3g"
          % float((err / np.maximum(lim, 1e-300)).max(initial=0.0)))
    assert (err <= lim).all(), what


def _check_stats(got, ref, tol, what):
    v = ref["vals"]
    n = len(v)
    assert got["nnz"] == int((np.abs(v) > tol).sum()), what
    assert got["active_features"] == ref["active"], what
    want_sq, want_abs = float(np.sum(v * v)), float(np.sum(np.abs(v)))
    e_sq = abs(got["sum_sq"] - want_sq) / want_sq if want_sq else abs(got["sum_sq"])
    e_abs = abs(got["sum_abs"] - want_abs) / want_abs if want_abs else abs(got["sum_abs"])
    print(what, "sum_sq, sum_abs relative errors %.3g %.3g, allowed %.3g" % (e_sq, e_abs, n * EPS))
    assert e_sq <= n * EPS and e_abs <= n * EPS, what
    top = int(np.argmax(np.abs(v))) if n else 0
    if n:
        assert abs(got["max_abs"] - abs(v[top])) <= (ref["k"] + 3) * EPS * ref["bound"][top], what
    else:
        assert got["max_abs"] == 0.0


# ------------------------------------------------------------------ blocks
def _random_block(seed, k, d, d_active, f32):
    """d_active of the d columns non-zero (interleaved), holes inside them, lams of both signs"""
    rng = np.random.RandomState(seed)
    P = rng.randn(k, d) + 0.1 * np.sign(rng.randn(k, d))
    P *= rng.rand(k, d) < 0.8
    dead = rng.permutation(d)[:d - d_active]
    P[:, dead] = 0.0
    alive = np.setdiff1d(np.arange(d), dead)
    P[0, alive] = np.where(P[0, alive] == 0, 0.2 + rng.rand(len(alive)), P[0, alive])  # all active
    if f32:
        P = P.astype(np.float32).astype(np.float64)
    lams = np.where(np.arange(k) % 2 == 0, -1.0, 1.0)
    return P, lams


SHAPES = {40: (40, 40), 70: (70, 70), 200: (260, 200)}  # d_a -> (d, d_a)


@functools.lru_cache(maxsize=None)
def _case(da, k, f32):
    d, d_active = SHAPES[da]
    P, lams = _random_block(1000 * da + k, k, d, d_active, f32)
    ref = _reference(P, lams)
    assert ref["active"] == da
    return P, lams, ref


def _live(P, lams, layout, precision):
    """what the handle of ``_engine(P, lams, layout, precision=...)`` holds (a twin's read-back)"""
    if layout == "P":
        return P
    twin = _engine(P, lams, layout, precision=precision)
    Pl, _ = twin.get_params()
    twin.close()
    return np.ascontiguousarray(Pl[0])


def _check_all(eng, ref, K, what):
    _preconditions(ref, K)
    _check_stats(eng.interaction3_stats(0, 0.0), ref, 0.0, (what, "stats"))
    sel = _select(ref)
    _check_triples(eng.interaction3_topk(0, K), ref, _top(ref, K), (what, "topk"))
    got = eng.interaction3_list(0, 0.0, len(sel["vals"]))
    _check_triples(got, sel, slice(None), (what, "list"))
    # a threshold in the widest gap around the median magnitude
    m = np.sort(np.abs(sel["vals"]))
    if len(m) >= 4:
        lo, hi = max(1, len(m) // 2 - 50), min(len(m) - 1, len(m) // 2 + 50)
        q = lo + int(np.argmax(m[lo:hi + 1] - m[lo - 1:hi]))
        tol = float(0.5 * (m[q - 1] + m[q]))
        _preconditions(ref, K, tol)
        _check_stats(eng.interaction3_stats(0, tol), ref, tol, (what, "stats tol"))
        st = _select(ref, tol)
        got = eng.interaction3_list(0, tol, len(st["vals"]))
        _check_triples(got, st, slice(None), (what, "list tol"))
    # values: the listed triples, ids permuted
    pick = np.arange(0, len(sel["vals"]), max(1, len(sel["vals"]) // 500))
    vals = eng.interaction3_values(0, sel["l"][pick], sel["i"][pick], sel["j"][pick])
    _check_triples((sel["i"][pick], sel["j"][pick], sel["l"][pick], vals), sel, pick,
                   (what, "values"))


# ------------------------------------------------------------------ 1. shapes, storage, layouts
@pytest.mark.parametrize("k", [1, 5, 37])
@pytest.mark.parametrize("da", [40, 70, 200])
def test_shapes(da, k):
    P, lams, ref = _case(da, k, False)
    eng = _engine(P, lams, "P")
    _check_all(eng, ref, 100, ("f64 P", da, k))
    eng.close()


@pytest.mark.parametrize("layout,precision", [("P", "f32"), ("Pt", "f32"), ("Pt", "f64")])
@pytest.mark.parametrize("da,k", [(70, 5), (200, 37)])
def test_storage_and_layouts(da, k, layout, precision):
    P, lams, ref = _case(da, k, precision == "f32")
    Pl = _live(P, lams, layout, precision)
    if not np.array_equal(Pl, P):  # the epoch behind layout "Pt" may move the last bits
        assert np.abs(Pl - P).max() <= 1e-6 * np.abs(P).max()
        ref = _reference(Pl, lams)
    eng = _engine(P, lams, layout, precision=precision)
    _check_all(eng, ref, 100, (precision, layout, da, k))
    got, _ = eng.get_params()
    assert np.array_equal(got[0], Pl)  # the handle held exactly the numbers of the reference
    eng.close()


# ------------------------------------------------------------------ 2. integer blocks: exact
def _integer_block(seed, k, d):
    rng = np.random.RandomState(seed)
    P = rng.randint(-2, 3, size=(k, d)).astype(np.float64)
    P *= rng.rand(k, d) < 0.35
    P[:, rng.rand(d) < 0.2] = 0.0
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    return P, lams


@pytest.mark.parametrize("layout", ["P", "Pt"])
@pytest.mark.parametrize("k,d", [(5, 150), (37, 70)])
def test_integer_blocks_exact(k, d, layout):
    P, lams = _integer_block(7 * k + d, k, d)
    ref = _reference(P, lams)  # sums of small integers: exact on both sides
    v = ref["vals"]
    assert (v == np.round(v)).all() and 0 < np.count_nonzero(v) < len(v)
    eng = _engine(P, lams, layout)
    for tol in (0.0, 1.0, 2.0):
        st = eng.interaction3_stats(0, tol)
        assert st == dict(nnz=int((np.abs(v) > tol).sum()), active_features=ref["active"],
                          sum_sq=float(np.sum(v * v)), sum_abs=float(np.sum(np.abs(v))),
                          max_abs=float(np.abs(v).max())), tol
        sel = _select(ref, tol)
        got = eng.interaction3_list(0, tol, st["nnz"])
        for a, b in zip(got, (sel["i"], sel["j"], sel["l"], sel["vals"])):
            assert np.array_equal(a, b)
    nnz = int(np.count_nonzero(v))
    for K in (1, 10, 333, nnz, nnz + 10):  # ties everywhere: the order is (|T| desc, i, j, l)
        idx = _top(ref, K)
        got = eng.interaction3_topk(0, K)
        assert len(got[3]) == min(K, nnz)
        for a, b in zip(got, (ref["i"][idx], ref["j"][idx], ref["l"][idx], v[idx])):
            assert np.array_equal(a, b), K
    li, lj, ll, lv = eng.interaction3_list(0, 0.0, nnz)
    perm = np.random.RandomState(0).randint(0, 6, size=nnz)
    ids = np.stack([li, lj, ll])
    orders = np.array([(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)])[perm]
    x, y, z = (ids[orders[:, c], np.arange(nnz)] for c in range(3))
    assert eng.interaction3_values(0, x, y, z).tobytes() == lv.tobytes()
    eng.close()


# ------------------------------------------------------------------ 3. determinism, budgets
def test_determinism_and_tile_budget():
    P, lams, ref = _case(200, 37, False)
    seen, units = None, 4 * 5 * 6 // 6  # T = 4 tiles: T (T + 1) (T + 2) / 6 units
    for budget in (1, 7, 0):
        eng = _engine(P, lams, "P", options={"interaction_tile_budget": budget})
        for _ in range(2):
            st = eng.interaction3_stats(0, 0.0)
            launches = eng.get_option("interaction_launches")
            top = eng.interaction3_topk(0, 1000)
            lst = eng.interaction3_list(0, 1.0, st["nnz"])
            blob = pickle.dumps((st, [a.tobytes() for a in top], [a.tobytes() for a in lst]))
            seen = seen or blob
            assert blob == seen, budget
        assert launches == {1: units, 7: -(-units // 7), 0: 1}[budget] and units > 1
        eng.close()


# ------------------------------------------------------------------ 4. errors and edges
def test_errors_and_edges():
    from sparsepoly_amd import _capi

    P, lams, ref = _case(70, 5, False)
    sel = _select(ref)
    n = len(sel["vals"])
    eng = _engine(P, lams)
    # K beyond the non-zero triples; K = 0; tol above max_abs
    got = eng.interaction3_topk(0, n + 1000)
    assert len(got[3]) == n
    assert all(len(a) == 0 for a in eng.interaction3_topk(0, 0))
    big = eng.interaction3_stats(0, 0.0)["max_abs"]
    st = eng.interaction3_stats(0, 2 * big)
    assert st["nnz"] == 0 and st["max_abs"] == big
    assert all(len(a) == 0 for a in eng.interaction3_list(0, 2 * big, 10))
    # short capacity: error, count reported, outputs untouched
    arrs = [np.full(n, -7, dtype=np.int32) for _ in range(3)]
    vals = np.full(n, -7.0)
    n_out = C.c_int64(-1)
    rc = eng._lib.spfm_interaction3_list(eng._h, 0, 0.0, n - 1,
                                         *[a.ctypes.data_as(_capi._ip) for a in arrs],
                                         vals.ctypes.data_as(_capi._dp), C.byref(n_out))
    assert rc == _capi.SPFM_ERR_INVALID and n_out.value == n
    assert str(n) in eng._lib.spfm_last_error(eng._h).decode()
    assert all((a == -7).all() for a in arrs) and (vals == -7.0).all()
    with pytest.raises(ValueError, match=str(n)):
        eng.interaction3_list(0, 0.0, n - 1)
    # invalid arguments
    for call in (lambda: eng.interaction3_stats(0, -1.0), lambda: eng.interaction3_topk(0, -1),
                 lambda: eng.interaction3_list(0, -1.0, 5), lambda: eng.interaction3_list(0, 0.0, -1),
                 lambda: eng.interaction3_stats(1, 0.0), lambda: eng.interaction3_stats(-1, 0.0),
                 lambda: eng.interaction3_values(0, [0], [1], [70]),
                 lambda: eng.interaction3_values(0, [-1], [1], [2])):
        with pytest.raises(ValueError):
            call()
    # values: repeated ids give 0, whichever two
    i, j, l = sel["i"][:50], sel["j"][:50], sel["l"][:50]
    for x, y, z in ((i, i, l), (i, l, l), (l, j, l), (i, i, i)):
        assert not eng.interaction3_values(0, x, y, z).any()
    assert eng.interaction3_values(0, [], [], []).shape == (0,)
    # interaction_features cuts off the last columns
    cut = _reference(P[:, :50], lams)
    st = eng.interaction3_stats(0, 0.0, n_features=50)
    _check_stats(st, cut, 0.0, "first 50 features")
    got = eng.interaction3_list(0, 0.0, st["nnz"], n_features=50)
    _check_triples(got, _select(cut), slice(None), "first 50 features, list")
    assert eng.get_option("interaction_features") == 0  # restored
    eng.close()
    # missing parameters
    from sparsepoly_amd.engine import HipEngine

    bare = HipEngine(0, "f64")
    with pytest.raises(ValueError, match="no parameters"):
        bare.interaction3_stats(0, 0.0)
    bare.close()


@pytest.mark.parametrize("active", [0, 1, 2])
def test_fewer_than_three_active_features(active):
    P = np.zeros((3, 20))
    P[:, [4, 11][:active]] = 1.5
    eng = _engine(P, np.ones(3))
    assert eng.interaction3_stats(0, 0.0) == dict(nnz=0, active_features=active, sum_sq=0.0,
                                                  sum_abs=0.0, max_abs=0.0)
    assert all(len(a) == 0 for a in eng.interaction3_topk(0, 5))
    assert all(len(a) == 0 for a in eng.interaction3_list(0, 0.0, 5))
    assert eng.interaction3_values(0, [4], [11], [0])[0] == 0.0
    eng.close()


def test_work_guard():
    from sparsepoly_amd import _capi

    d = _capi.INTERACTION3_MAX_ACTIVE + 1
    P = np.ones((1, d))
    eng = _engine(P, np.ones(1))
    small = eng.interaction3_stats(0, 0.0, n_features=10)
    assert small["nnz"] == 120
    launches = eng.get_option("interaction_launches")
    assert launches >= 1
    for call in (lambda: eng.interaction3_stats(0, 0.0), lambda: eng.interaction3_topk(0, 5),
                 lambda: eng.interaction3_list(0, 0.0, 5)):
        with pytest.raises(NotImplementedError, match=r"d_a = %d .*interaction_features" % d):
            call()
        assert eng.get_option("interaction_launches") == launches  # refused before any pass
    rc = eng._lib.spfm_interaction3_stats(eng._h, 0, 0.0, (C.c_int64 * 2)(), (C.c_double * 3)())
    assert rc == _capi.SPFM_ERR_UNSUPPORTED
    assert eng.interaction3_values(0, [0], [d - 1], [5])[0] == 1.0  # values has no guard
    eng.close()


# ------------------------------------------------------------------ 5. read-only
def _probe3(eng, o):
    st = eng.interaction3_stats(o, 0.0)
    eng.interaction3_topk(o, 10)
    eng.interaction3_list(o, 0.0, st["nnz"])
    eng.interaction3_values(o, [0, 1], [5, 6], [7, 8])


def test_read_only():
    """``get_params`` bit-equal around the calls; the pcd epochs after them give the bits of a
    run without them; the pair entries give the same bits before and after a triple pass (they
    share the scratch)."""
    X, y = _problem(300, 40, 6, 3)
    out = []
    for probing in (True, False):
        run = _Live(X, y, *LIVE["pcd_omegati3"], precision="f32")

        def probe(r):
            before = r.eng.get_params()  # the same reads in both runs
            if probing:
                pair = (r.eng.interaction_stats(1, 0.0),
                        [a.tobytes() for a in r.eng.interaction_topk(1, 20)])
                _probe3(r.eng, 0)
                assert pair == (r.eng.interaction_stats(1, 0.0),
                                [a.tobytes() for a in r.eng.interaction_topk(1, 20)])
            after = r.eng.get_params()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

        for _ in range(2):
            run.iterate(probe)
        P, w = run.eng.get_params()
        out.append((P, w, run.eng.get_y_pred(), np.array(run.viol), run.flags))
        assert np.any(P != run.P0)
        run.eng.close()
    a, b = out
    for q in range(4):
        assert np.array_equal(a[q], b[q]), q
    assert a[4] == b[4]


# ------------------------------------------------------------------ 6. estimators
def _check_estimator(est, P, lams, **kw):
    ref = _reference(P, lams)
    _preconditions(ref, 20)
    sel = _select(ref)
    _check_stats(est.triple_stats(**kw), ref, 0.0, "estimator stats")
    _check_triples(est.top_triples(20, **kw), ref, _top(ref, 20), "estimator top")
    got = est.triples(**kw)
    _check_triples(got, sel, slice(None), "estimator list")
    n = len(sel["vals"])
    if n:
        with pytest.raises(ValueError, match=str(n)):
            est.triples(max_triples=n - 1, **kw)
        vals = est.triple_values(got[2][:30], got[0][:30], got[1][:30], **kw)
        _check_triples((got[0][:30], got[1][:30], got[2][:30], vals), sel, slice(0, 30), "values")
    return ref, n


def test_degree3_omegati_regressor_with_monitor():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.interactions import support_recovery3
    from sparsepoly_amd.monitor import Monitor

    X, y = _problem(300, 30, 6, 4)
    counts = []

    class Probe(Monitor):
        def __call__(self, est):
            counts.append(est.triple_stats()["nnz"])
            return Monitor.__call__(self, est)

    est = SparseFactorizationMachineRegressor(
        degree=3, n_components=4, solver="pcd", regularizer="omegati", beta=1.0, gamma=1e-3,
        max_iter=3, tol=-1, n_calls=1, callback=Probe(), random_state=0, precision="f64")
    with _quiet():
        est.fit(X, y)
    ref, n = _check_estimator(est, est.P_[0], est.lams_)  # order 0 holds the degree-3 block
    assert len(counts) >= 3 and counts[-1] == n and n > 0
    r = support_recovery3(est, (ref["i"][:40], ref["l"][:40], ref["j"][:40]))
    tp = int(np.count_nonzero(ref["vals"][:40]))
    assert (r["nnz"], r["tp"], r["fn"], r["fp"]) == (n, tp, 40 - tp, n - tp)


def test_all_subsets_regressor():
    from sparsepoly_amd import SparseAllSubsetsRegressor

    X, y = _problem(300, 30, 6, 4)
    est = SparseAllSubsetsRegressor(n_components=4, solver="pcd", regularizer="omegati", beta=1.0,
                                    gamma=1e-2, max_iter=3, tol=-1, random_state=0,
                                    precision="f64")
    with _quiet():
        est.fit(X, y)
    _, n = _check_estimator(est, est.P_, est.lams_)
    assert n > 0


def test_include_augmented():
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y = _problem(300, 30, 6, 4)
    est = SparseFactorizationMachineRegressor(
        degree=3, n_components=4, solver="pcd", regularizer="l1", fit_lower="augment",
        fit_linear=False, beta=1e-3, gamma=1e-3, max_iter=3, tol=-1, random_state=0,
        precision="f64")
    with _quiet():
        est.fit(X, y)
    P = est.P_[0]
    assert P.shape == (4, 32) and P[:, 30:].any()  # two dummy columns after the 30 features
    _, n_real = _check_estimator(est, P[:, :30], est.lams_)
    _, n_all = _check_estimator(est, P, est.lams_, include_augmented=True)
    assert n_all > n_real
    assert est.triples()[2].max() < 30 <= est.triples(include_augmented=True)[2].max()
    assert est.triple_values([0], [1], [31], include_augmented=True).shape == (1,)
    with pytest.raises(ValueError, match="out of range"):
        est.triple_values([0], [1], [31])
