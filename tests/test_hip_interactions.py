"""``spfm_interaction_*`` and what the estimators build on them, on the device.  Needs a real
MI355X: ``pytest -m gpu``.

The device values are compared with the dense NumPy restatement of
``tests/test_interactions_host.py`` (itself pinned to the metrics recorded from the reference
there).  Bounds, all from the arithmetic and none from a device run:

* one entry of W is a dot product of length k; in any summation order, fused or not, its forward
  error is at most ``(k + 2) 2^-53 sum_s |p_sj p_sj'|``.  The device value is held to exactly
  that bound against a restatement in ``np.longdouble`` (``restate(..., wide=True)``), whose own
  error, 2^-11 of the bound, is covered by the 2 in ``k + 2`` (a dot product needs ``k``);
* sums over entries: that bound summed over the entries, nothing added (for ``sum W^2`` the
  bound ``e`` of an entry turns into ``(2 |w| + e) e``).  Each figure is printed as a fraction
  of its bound before it is asserted;
* counts, index lists and orders are exact.  Thresholds and ties are where a device run could
  legitimately differ, so every case asserts ON THE NUMPY SIDE, before the device is touched,
  that no ``|W|`` lies within ``1e-9 max|W|`` of the threshold (for ``tol = 0``: no entry with a
  non-zero term is that small, nor smaller than four times its own error bound) and that the
  top K + 1 magnitudes are that far apart.  No case is skipped for failing it: the seeds below
  pass it (checked on the CPU).
"""
import contextlib
import pickle
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import load_golden
from test_hip_objective import LIVE, _Live, _problem
from test_interactions_host import FITS, restate, restate_metrics

pytestmark = pytest.mark.gpu

@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield


U = 2.0 ** -53
CLEAR = 1e-9  # relative distance every threshold / tie keeps (see the module docstring)


def _engine(P, lams, layout="P", options=None, precision="f64"):
    """A handle holding a block (k, d): after ``set_params`` only (layout "P": the (k,d) image
    is live and holds P), or after one pbcd epoch with step size 0 and no penalty on a one-entry
    matrix (layout "Pt": the (d,k) image is live).  What that image holds is read back from a
    twin handle by ``_live_block``; epochs are bit-reproducible from handle to handle, and every
    caller asserts afterwards that its own handle held exactly those numbers."""
    from sparsepoly_amd.engine import HipEngine

    k, d = P.shape
    eng = HipEngine(0, precision)
    for key, val in (options or {}).items():
        eng.set_option(key, val)
    if layout == "Pt":
        X = sp.csr_matrix((np.ones(1), (np.zeros(1, dtype=int), np.zeros(1, dtype=int))),
                          shape=(1, d))
        eng.set_data(X, np.zeros(1))
    eng.set_params(P[None], np.zeros(d), lams)
    if layout == "Pt":
        eng.configure("pbcd", "squared", "l21", 2)
        eng.init_pred(2, False, False)
        eng.set_schedule("exact", np.arange(d, dtype=np.int32))
        eng.pbcd_epoch(0, 2, 1.0, 0.0, 0.0)
    return eng


def _live_block(P, lams, layout):
    """The numbers the handle of ``_engine(P, lams, layout)`` holds, as a host array: P itself,
    or the result of the same set-up on a twin handle (so that the NumPy side of a case, with its
    preconditions, is complete before the handle under test is touched)."""
    if layout == "P":
        return P
    twin = _engine(P, lams, layout)
    Pl, _ = twin.get_params()
    twin.close()
    assert np.abs(Pl[0] - P).max(initial=0.0) <= 1e-12 * np.abs(P).max(initial=1.0)
    return np.ascontiguousarray(Pl[0])


def _block(seed, k, d, sparsity):
    """Random block with `sparsity` of its columns zero (1.0: all), entries of one sign per
    component on the support, random +-1 lams."""
    rng = np.random.RandomState(seed)
    P = np.abs(rng.randn(k, d)) + 0.05
    P *= np.where(rng.rand(k, 1) < 0.5, -1.0, 1.0)
    P *= rng.rand(k, d) < 0.7  # holes inside the active columns
    if sparsity >= 1.0:
        P[:] = 0.0
    elif sparsity > 0.0:
        P[:, rng.rand(d) < sparsity] = 0.0
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    return P, lams


def _plan(P, lams, K):
    """The NumPy side of one case, with the preconditions asserted: -> (restatement at tol 0,
    tol > 0, restatement at that tol)."""
    k = P.shape[0]
    r0 = restate(P, lams, 0.0, top=K + 1, wide=True)
    iu = np.triu_indices(P.shape[1], k=1)
    we, bd = np.abs(r0["W"][iu]), r0["bound"][iu]
    big = r0["max_abs"]
    live = bd > 0  # pairs with any non-zero term
    if live.any():
        assert we[live].min() > CLEAR * big, "tol = 0: an entry too close to zero"
        assert (we[live] > 4 * (k + 2) * U * bd[live]).all(), "tol = 0: entry within its error"
    assert not we[~live].any()
    mags = np.abs(r0["top_vals"])
    if len(mags) > 1:
        assert np.diff(-mags).min() > CLEAR * big, "top K + 1 magnitudes too close"
    tol, rt = 0.0, None
    m = np.sort(we[live])
    if len(m) >= 4:
        lo, hi = max(1, len(m) // 2 - 50), min(len(m) - 1, len(m) // 2 + 50)
        i = lo + int(np.argmax(m[lo:hi + 1] - m[lo - 1:hi]))
        tol = float(0.5 * (m[i - 1] + m[i]))
        assert m[i] - tol > CLEAR * big and tol - m[i - 1] > CLEAR * big, "tol too close"
        rt = restate(P, lams, float(tol), top=K + 1, wide=True)
    return r0, tol, rt


def _check_stats(got, want, k, what):
    """``want``: a ``restate(..., wide=True)``"""
    assert want["W"].dtype == np.longdouble
    assert got["nnz"] == want["nnz"], (what, got, want["nnz"])
    assert got["active_features"] == want["active_features"], what
    iu = np.triu_indices(want["W"].shape[0], k=1)
    bd, we = want["bound"][iu].astype(np.longdouble), np.abs(want["W"][iu])
    e = (k + 2) * U * bd  # per entry; d(w^2) <= (2 |w| + e) e
    tols = dict(sum_abs=e.sum(), sum_sq=((2 * we + e) * e).sum(), max_abs=e.max(initial=0.0))
    errs = {key: abs(np.longdouble(got[key]) - want[key]) for key in tols}
    print(what, {key: "%.3g of its bound" % float(errs[key] / tols[key])
                 for key in tols if tols[key] > 0})
    for key in tols:
        assert errs[key] <= tols[key], (what, key, got[key], want[key], float(tols[key]))


def _check_pairs(rows, cols, vals, want_rows, want_cols, want_vals, bound, k, what):
    np.testing.assert_array_equal(rows, want_rows, err_msg=str(what))
    np.testing.assert_array_equal(cols, want_cols, err_msg=str(what))
    assert rows.dtype == np.int32 and cols.dtype == np.int32
    tol = (k + 2) * U * bound[want_rows, want_cols]
    err = np.abs(vals.astype(np.longdouble) - want_vals)
    assert (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()))


def _check_all(eng, P, lams, K, plan, what):
    k = P.shape[0]
    r0, tol, rt = plan
    _check_stats(eng.interaction_stats(0, 0.0), r0, k, (what, "stats"))
    rows, cols, vals = eng.interaction_topk(0, K)
    n = min(K, r0["nnz"])
    _check_pairs(rows, cols, vals, r0["top_rows"][:n], r0["top_cols"][:n], r0["top_vals"][:n],
                 r0["bound"], k, (what, "topk"))
    rows, cols, vals = eng.interaction_list(0, 0.0, r0["nnz"])
    _check_pairs(rows, cols, vals, r0["rows"], r0["cols"], r0["vals"], r0["bound"], k,
                 (what, "list"))
    if rt is not None:
        _check_stats(eng.interaction_stats(0, tol), rt, k, (what, "stats tol"))
        rows, cols, vals = eng.interaction_list(0, tol, rt["nnz"])
        _check_pairs(rows, cols, vals, rt["rows"], rt["cols"], rt["vals"], rt["bound"], k,
                     (what, "list tol"))


# ------------------------------------------------------------------ 1. fixture parity
@pytest.mark.parametrize("layout", ["P", "Pt"])
@pytest.mark.parametrize("name", FITS)
def test_fixture_parity(name, layout):
    z = load_golden("g12_interactions.npz")
    P, lams = np.ascontiguousarray(z[name + "_P"]), z[name + "_lams"]
    k = P.shape[0]
    Pw = _live_block(P, lams, layout)
    r = restate(Pw, lams, 0.0, top=50, wide=True)  # values: wider than the fixture's float64
    eng = _engine(P, lams, layout)
    got = eng.interaction_stats(0, 0.0)
    assert got["nnz"] == int(z[name + "_nnz"])
    _check_stats(got, r, k, name)
    rows, cols, vals = eng.interaction_list(0, 0.0, got["nnz"])
    _check_pairs(rows, cols, vals, z[name + "_rows"], z[name + "_cols"], r["vals"],
                 r["bound"], k, name)
    rows, cols, vals = eng.interaction_topk(0, 50)
    _check_pairs(rows, cols, vals, z[name + "_top_rows"], z[name + "_top_cols"],
                 r["top_vals"], r["bound"], k, name)
    Pl, _ = eng.get_params()
    assert np.array_equal(Pl[0], Pw)
    eng.close()


# ------------------------------------------------------------------ 2. random blocks
DS = (1, 2, 15, 16, 17, 63, 64, 65, 1000, 3001)
KS = (1, 3, 4, 5, 30, 31, 64, 256)
SPARSITY = (0.0, 0.5, 0.99, 1.0)


def _seed(d, k, si):
    return 1000 * DS.index(d) + 10 * KS.index(k) + si


@pytest.mark.parametrize("d", DS)
def test_random_blocks(d):
    K = 20
    for k in KS:
        for si, sparsity in enumerate(SPARSITY):
            P, lams = _block(_seed(d, k, si), k, d, sparsity)
            plan = _plan(P, lams, K)  # preconditions asserted here, before any device call
            for layout in ("P", "Pt"):
                Pw = _live_block(P, lams, layout)
                if Pw is not P and not np.array_equal(Pw, P):
                    plan = _plan(Pw, lams, K)
                eng = _engine(P, lams, layout)
                _check_all(eng, Pw, lams, K, plan, (d, k, sparsity, layout))
                Pl, _ = eng.get_params()
                assert np.array_equal(Pl[0], Pw), (d, k, sparsity, layout)
                eng.close()


# ------------------------------------------------------------------ 3. ties
def test_ties_exact_order():
    rng = np.random.RandomState(5)
    k, d = 6, 150
    P = rng.randint(-2, 3, size=(k, d)).astype(np.double)
    P[:, rng.rand(d) < 0.3] = 0.0
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    r = restate(P, lams, 0.0, top=400)  # small integers: exact in any order
    mags = np.abs(r["top_vals"])
    assert len(mags) == 400 and len(np.unique(mags)) < 12  # many equal |W|
    for layout in ("P", "Pt"):
        assert np.array_equal(_live_block(P, lams, layout), P)
        eng = _engine(P, lams, layout)
        for K in (1, 7, 64, 400):
            rows, cols, vals = eng.interaction_topk(0, K)
            np.testing.assert_array_equal(rows, r["top_rows"][:K])
            np.testing.assert_array_equal(cols, r["top_cols"][:K])
            np.testing.assert_array_equal(vals, r["top_vals"][:K])
        got = eng.interaction_stats(0, 0.0)
        assert (got["nnz"], got["sum_sq"], got["sum_abs"], got["max_abs"]) == (
            r["nnz"], r["sum_sq"], r["sum_abs"], r["max_abs"])
        for tol in (0.0, 1.0, 2.5):
            rt = restate(P, lams, tol)
            rows, cols, vals = eng.interaction_list(0, tol, rt["nnz"])
            np.testing.assert_array_equal(rows, rt["rows"])
            np.testing.assert_array_equal(cols, rt["cols"])
            np.testing.assert_array_equal(vals, rt["vals"])
            assert eng.interaction_stats(0, tol)["nnz"] == rt["nnz"]
        # more pairs than asked for exist, fewer than asked for exist
        rows, _, _ = eng.interaction_topk(0, r["nnz"] + 10)
        assert len(rows) == r["nnz"]
        eng.close()


# ------------------------------------------------------------------ 4. determinism
def test_determinism_and_tile_budget():
    P, lams = _block(77, 30, 3001, 0.0)
    seen = None
    for budget in (0, 16):
        eng = _engine(P, lams, "P", options={"interaction_tile_budget": budget})
        for _ in range(3):
            st = eng.interaction_stats(0, 0.0)
            launches = eng.get_option("interaction_launches")
            top = eng.interaction_topk(0, 1000)
            lst = eng.interaction_list(0, 1.0, st["nnz"])
            blob = pickle.dumps((st, [a.tobytes() for a in top], [a.tobytes() for a in lst]))
            seen = seen or blob
            assert blob == seen, budget
        assert st["active_features"] == 3001
        assert launches >= 50 if budget else launches == 1
        eng.close()


# ------------------------------------------------------------------ 5. nothing of size d_a^2
def test_no_dense_product_at_200k_features():
    d, k = 200_000, 8
    rng = np.random.RandomState(11)
    v = 0.5 + rng.rand(d)
    lams = np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, -1.0])
    P = np.zeros((k, d))
    P[np.arange(d) % k, np.arange(d)] = v
    # closed forms, O(d log d): W[j, j'] = lams[s] v_j v_j' inside component s, 0 across
    # (sums in np.longdouble, like the wide restatement of the other tests)
    nnz, sum_sq, sum_abs, cand = 0, np.longdouble(0), np.longdouble(0), []
    for s in range(k):
        js = np.arange(s, d, k)
        vs = v[js]
        vl = vs.astype(np.longdouble)
        nnz += len(js) * (len(js) - 1) // 2
        sum_sq += (np.sum(vl ** 2) ** 2 - np.sum(vl ** 4)) / 2
        sum_abs += (np.sum(vl) ** 2 - np.sum(vl ** 2)) / 2
        top = js[np.argsort(-vs, kind="stable")[:101]]  # the top 100 products use these only
        a, b = np.triu_indices(len(top), k=1)
        r_, c_ = np.minimum(top[a], top[b]), np.maximum(top[a], top[b])
        cand += list(zip(-(v[r_] * v[c_]), r_, c_, lams[s] * (v[r_] * v[c_])))
    cand.sort()
    cand = cand[:101]
    mags = -np.array([c[0] for c in cand])
    assert np.diff(-mags).min() > 0  # single products: exact on both sides, ties excluded here
    eng = _engine(P, lams, "P")
    free0 = eng.get_option("free_mem_mib")
    st = eng.interaction_stats(0, 0.0)
    rows, cols, vals = eng.interaction_topk(0, 100)
    free1 = eng.get_option("free_mem_mib")
    assert st["nnz"] == nnz and st["active_features"] == d
    # every entry is one product, so its bound sum_s |p_sj p_sj'| is |W| itself: the summed bounds
    # are (k + 2) 2^-53 sum |W| and, for the squares, (2 |w| + e) e summed = (2 + e') e' sum W^2
    e = (k + 2) * U
    errs = (abs(np.longdouble(st["sum_abs"]) - sum_abs) / (e * sum_abs),
            abs(np.longdouble(st["sum_sq"]) - sum_sq) / ((2 + e) * e * sum_sq))
    print("200k: sum_abs, sum_sq errors as fractions of their bounds: %.3g %.3g"
          % (float(errs[0]), float(errs[1])))
    assert errs[0] <= 1 and errs[1] <= 1
    assert st["max_abs"] == mags[0]
    np.testing.assert_array_equal(rows, [c[1] for c in cand[:100]])
    np.testing.assert_array_equal(cols, [c[2] for c in cand[:100]])
    np.testing.assert_array_equal(vals, [c[3] for c in cand[:100]])
    # A dense W would be 320 GB; the scratch the entries hold and the drop of free device memory
    # over the calls stay under 1 GiB.  Free memory is sampled before and after the calls, not
    # during them: that bounds the peak only because every scratch buffer stays allocated on the
    # handle until spfm_set_params / "interaction_release" (the rocprim temporaries included; the
    # candidate vectors on the host are no device memory).  A change that frees scratch inside a
    # call has to move this check to a sample taken during the call.
    assert eng.get_option("interaction_scratch_kib") < (1 << 20)
    assert free0 - free1 < 1024, (free0, free1)
    assert eng.get_option("interaction_scratch_kib") > 0
    eng.release_interaction_scratch()
    assert eng.get_option("interaction_scratch_kib") == 0
    assert eng.interaction_stats(0, 0.0) == st  # and the next call allocates again: same bits
    eng.close()


# ------------------------------------------------------------------ 6. capacity
def test_capacity():
    import ctypes as C

    from sparsepoly_amd import SparseFactorizationMachineRegressor, _capi

    P, lams = _block(3, 5, 65, 0.0)
    n = restate(P, lams)["nnz"]
    assert n > 10
    eng = _engine(P, lams)
    rows = np.full(n, -7, dtype=np.int32)
    cols = np.full(n, -7, dtype=np.int32)
    vals = np.full(n, -7.0)
    n_out = C.c_int64(-1)
    rc = eng._lib.spfm_interaction_list(eng._h, 0, 0.0, n - 1, rows.ctypes.data_as(_capi._ip),
                                        cols.ctypes.data_as(_capi._ip),
                                        vals.ctypes.data_as(_capi._dp), C.byref(n_out))
    assert rc == _capi.SPFM_ERR_INVALID and n_out.value == n
    assert str(n) in eng._lib.spfm_last_error(eng._h).decode()
    assert (rows == -7).all() and (cols == -7).all() and (vals == -7.0).all()
    with pytest.raises(ValueError, match=str(n)):
        eng.interaction_list(0, 0.0, n - 1)
    eng.close()
    est = SparseFactorizationMachineRegressor(degree=2, n_components=5, fit_linear=False)
    est.P_, est.lams_, est.w_ = P[None], lams, np.zeros(65)
    with pytest.raises(ValueError, match=str(n)):
        est.interactions(max_pairs=n - 1)
    assert est.interactions(max_pairs=n).nnz == n


# ------------------------------------------------------------------ 7. read-only
def _probe_engine(eng, o):
    st = eng.interaction_stats(o, 0.0)
    eng.interaction_topk(o, 10)
    eng.interaction_list(o, 0.0, st["nnz"])
    eng.interaction_block(o, [0, 1, 2], [2, 3])
    eng.interaction_values(o, [0, 1], [5, 6])


@pytest.mark.parametrize("case", ["pcd_sql12", "pbcd_l21", "all_pcd"])
def test_read_only(case):
    X, y = _problem(2000, 150, 8, 7)
    out = []
    for probing in (True, False):
        run = _Live(X, y, *LIVE[case], precision="f32")
        o = run.blocks()[0][0]

        def probe(r):
            _probe_engine(r.eng, o)

        for _ in range(3):
            run.iterate(probe if probing else None)
        P, w = run.eng.get_params()
        out.append((P, w, run.eng.get_y_pred(), np.array(run.viol), run.flags))
        run.eng.close()
    a, b = out
    for i in range(4):
        assert np.array_equal(a[i], b[i]), (case, i)
    assert a[4] == b[4]


# psgd sums the gradient of a minibatch with hardware f64 atomics (spfm_psgd.hip.h,
# tests/test_hip_psgd.py): where three or more rows of a minibatch meet in one column the order of
# the additions is not fixed, and two runs of one problem differ in the last bit with or without a
# probe (measured on an MI355X, 2000 x 150, minibatches of 64, three epochs: plain against plain
# max|dP| = 1.388e-17 in 46 entries, plain against probed 1.388e-17 in 68).  A comparison of two
# runs bit for bit therefore says something about the probes only where training itself is
# reproducible: minibatches of ONE row, whose duplicate-free column list sends at most one addend
# to every address.  That is what the two-run psgd cases below use; any write of a probe into the
# parameters, the gradient buffers, the step counter or the prox state would still show.
PSGD_BATCH = 1


def test_read_only_psgd():
    """Two psgd runs on a g3-sized problem (300 x 60), one probed between all epochs:
    bit-identical parameters, loss sums and step counter (see ``PSGD_BATCH``)."""
    from sparsepoly_amd.engine import HipEngine

    X, y = _problem(300, 60, 8, 5)
    out = []
    for probing in (True, False):
        eng = HipEngine(0, "f32")
        eng.set_data(X, y)
        eng.set_params(0.05 * np.random.RandomState(2).randn(1, 5, 60), np.zeros(60), np.ones(5))
        eng.configure("psgd", "squared", "squaredl12", 2)
        it, losses = 1, []
        for _ in range(3):
            sl, it = eng.psgd_epoch(2, 1e-2, 0.1, 1e-3, 0.05, "optimal", 1.0, PSGD_BATCH,
                                    np.arange(300, dtype=np.int32), True, it)
            losses.append(sl)
            if probing:
                _probe_engine(eng, 0)
        P, w = eng.get_params()
        out.append((P, w, np.array(losses), it))
        eng.close()
    assert np.any(out[0][0] != 0.05 * np.random.RandomState(2).randn(1, 5, 60))  # it trained
    for i in range(3):
        assert np.array_equal(out[0][i], out[1][i]), i
    assert out[0][3] == out[1][3]


def test_read_only_psgd_same_handle():
    """Minibatches of 64, where two runs cannot be compared bit for bit (``PSGD_BATCH``): on ONE
    handle, the probes between two reads of the live state change nothing (both layouts: the
    (d,k) image the epochs leave, and the (k,d) image after ``get_params``), and the engine
    choices stay."""
    from sparsepoly_amd.engine import HipEngine

    X, y = _problem(2000, 150, 10, 5)
    eng = HipEngine(0, "f32")
    eng.set_data(X, y)
    eng.set_params(0.05 * np.random.RandomState(2).randn(1, 5, 150), np.zeros(150), np.ones(5))
    eng.configure("psgd", "squared", "squaredl12", 2)
    it = 1
    for _ in range(3):
        _, it = eng.psgd_epoch(2, 1e-2, 0.1, 1e-3, 0.05, "optimal", 1.0, 64,
                               np.arange(2000, dtype=np.int32), True, it)
        st_dk = eng.interaction_stats(0, 0.0)   # reads the (d,k) image
        _probe_engine(eng, 0)
        P0, w0 = eng.get_params()
        st_kd = eng.interaction_stats(0, 0.0)   # the (k,d) image is valid now: same bits
        assert st_kd == st_dk
        _probe_engine(eng, 0)
        P1, w1 = eng.get_params()
        assert np.array_equal(P0, P1) and np.array_equal(w0, w1)
        r = restate(P0[0], np.ones(5))
        assert st_dk["nnz"] == r["nnz"] and st_dk["active_features"] == r["active_features"]
    assert eng.get_option("psgd_redone") == 0
    eng.close()


@pytest.mark.parametrize("solver,reg", [("pcd", "squaredl12"), ("pbcd", "squaredl21"),
                                        ("psgd", "squaredl12"), ("all-subsets", "omegati")])
def test_read_only_estimator_callback(solver, reg, capsys):
    """Two fits, one with a callback that calls all four methods every iteration: bit-identical
    ``P_``, ``w_`` and per-iteration violation sums / epoch losses (the ``verbose`` lines, which
    print them in full; psgd: one-row minibatches on a g3-sized problem, see ``PSGD_BATCH``)."""
    from sparsepoly_amd import SparseAllSubsetsRegressor, SparseFactorizationMachineRegressor

    X, y = _problem(300, 60, 8, 9) if solver == "psgd" else _problem(1000, 100, 8, 9)
    fits, logs = [], []
    for probing in (True, False):
        def cb(est):
            if probing:
                st = est.interaction_stats()
                est.top_interactions(5)
                assert est.interactions().nnz == st["nnz"]
                est.interaction_block([0, 1, 2])

        if solver == "all-subsets":
            est = SparseAllSubsetsRegressor(
                n_components=4, solver="pcd", regularizer=reg, beta=1.0, gamma=1e-3, max_iter=4,
                tol=-1, n_calls=1, callback=cb, random_state=0, verbose=True)
        else:
            est = SparseFactorizationMachineRegressor(
                degree=2, n_components=4, solver=solver, regularizer=reg, beta=1.0, gamma=1e-3,
                max_iter=4, tol=-1, n_calls=1, callback=cb, random_state=0,
                batch_size=PSGD_BATCH, eta0=0.05, n_iter_no_change=100, verbose=True)
        capsys.readouterr()
        with _quiet():
            est.fit(X, y)
        logs.append(capsys.readouterr().out)
        fits.append(est)
    assert np.array_equal(fits[0].P_, fits[1].P_)
    if solver != "all-subsets":
        assert np.array_equal(fits[0].w_, fits[1].w_)
    assert logs[0].count("\n") >= 4 and logs[0] == logs[1]


# ------------------------------------------------------------------ 8. estimator level
def _metrics_equal(est, P, lams, W_true):
    from sparsepoly_amd.interactions import estimation_error, support_recovery

    m = restate_metrics(P, lams, W_true)
    got = support_recovery(est, W_true)
    for key in ("nnz", "tp", "fp", "fn", "pssr"):
        assert got[key] == m[key], (key, got, m)
    assert abs(got["fscore"] - m["fscore"]) <= 1e-12
    err = estimation_error(est, W_true)
    assert abs(err - m["error"]) <= 1e-12 * m["error"], (err, m["error"])
    err = estimation_error(est, sp.csr_matrix(W_true), scaling=False)
    assert abs(err - m["error_unscaled"]) <= 1e-12 * m["error_unscaled"]


def _notebook_fm(**kw):
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    args = dict(n_components=30, fit_linear=False, beta=0.2, gamma=0.1, regularizer="squaredl12",
                solver="pcd", mean=True, max_iter=30, tol=1e-3, random_state=0,
                precision="f64", schedule="exact")
    args.update(kw)
    return SparseFactorizationMachineRegressor(**args)


def test_estimator_on_the_notebook_data():
    z = load_golden("g12_interactions.npz")
    X, y, W_true = z["X"], z["y"], z["W_true"]
    est = _notebook_fm()
    with _quiet():
        est.fit(X, y)
    _metrics_equal(est, est.P_[0], est.lams_, W_true)
    st = est.interaction_stats()
    assert 0 < st["nnz"] < 4950  # squaredl12 selected a strict subset of the pairs
    W = est.interactions()
    r = restate(est.P_[0], est.lams_)
    assert W.shape == (100, 100) and W.nnz == r["nnz"]
    np.testing.assert_array_equal(W.row, r["rows"])
    np.testing.assert_array_equal(W.col, r["cols"])
    # a pickled and reloaded estimator has no session: a fresh engine answers the same
    again = pickle.loads(pickle.dumps(est))
    assert again.interaction_stats() == st
    a, b = est.top_interactions(50), again.top_interactions(50)
    assert all(np.array_equal(x, y_) for x, y_ in zip(a, b))
    # a kept warm_start session answers without a fresh engine, with the same bits
    warm = _notebook_fm(warm_start=True)
    with _quiet():
        warm.fit(X, y)
    assert getattr(warm, "_device_session", None) is not None
    assert np.array_equal(warm.P_, est.P_) and warm.interaction_stats() == st
    warm.release_device()


def test_mid_fit_call_under_pbcd_sees_the_live_block():
    z = load_golden("g12_interactions.npz")
    X, y, W_true = z["X"], z["y"], z["W_true"]
    seen = []

    def cb(est):
        eng = est._live[0]
        st = est.interaction_stats()
        rows, cols, vals = est.interactions().row, est.interactions().col, est.interactions().data
        P_live, _ = eng.get_params()
        seen.append((st, rows, cols, vals, P_live[0].copy(), est.P_[0].copy()))

    est = _notebook_fm(solver="pbcd", regularizer="squaredl21", gamma=1.0, max_iter=6, n_calls=1,
                       callback=cb)
    with _quiet():
        est.fit(X, y)
    assert len(seen) >= 3
    st, rows, cols, vals, P_live, P_stale = seen[2]
    assert not np.array_equal(P_live, P_stale)  # the fit loop does not refresh P_ under pbcd
    live, stale = restate(P_live, est.lams_, wide=True), restate(P_stale, est.lams_)
    assert st["nnz"] == live["nnz"]
    np.testing.assert_array_equal(rows, live["rows"])
    np.testing.assert_array_equal(cols, live["cols"])
    tol = (30 + 2) * U * live["bound"][rows, cols]
    assert (np.abs(vals.astype(np.longdouble) - live["vals"]) <= tol).all()
    _check_stats(st, live, 30, "mid-fit pbcd")
    assert abs(st["sum_sq"] - stale["sum_sq"]) > 1e-6 * stale["sum_sq"]


def test_include_augmented():
    z = load_golden("g12_interactions.npz")
    X, y = z["X"], z["y"]
    est = _notebook_fm(fit_lower="augment", max_iter=10)
    with _quiet():
        est.fit(X, y)
    P = est.P_[0]
    assert P.shape == (30, 101)
    for flag, Pv in ((False, P[:, :100]), (True, P)):
        r = restate(Pv, est.lams_)
        st = est.interaction_stats(include_augmented=flag)
        assert (st["nnz"], st["active_features"]) == (r["nnz"], r["active_features"])
        W = est.interactions(include_augmented=flag)
        assert W.shape == (Pv.shape[1],) * 2
        np.testing.assert_array_equal(W.row, r["rows"])
        np.testing.assert_array_equal(W.col, r["cols"])
        rows, cols, _ = est.top_interactions(30, include_augmented=flag)
        np.testing.assert_array_equal(rows, r["top_rows"][:30])
        np.testing.assert_array_equal(cols, r["top_cols"][:30])
    assert est.interaction_block([100], [0, 1], include_augmented=True).shape == (1, 2)
    with pytest.raises(ValueError, match="out of range"):
        est.interaction_block([100], [0, 1])


def test_monitor_records_interactions():
    from sparsepoly_amd.monitor import Monitor

    z = load_golden("g12_interactions.npz")
    counts = []

    class Both(Monitor):
        def __call__(self, est):
            counts.append(est.interaction_stats(self.interaction_tol)["nnz"])
            return Monitor.__call__(self, est)

    mon = Both(interactions=True, interaction_tol=1e-3)
    est = _notebook_fm(max_iter=5, n_calls=1, callback=mon)
    with _quiet():
        est.fit(z["X"], z["y"])
    assert len(mon.history) >= 4
    assert [rec["nnz_interactions"] for rec in mon.history] == counts
    # the last record was taken after the last epoch: the count of the fitted P_, restated
    r = restate(est.P_[0], est.lams_, 1e-3, wide=True)
    mags = np.abs(r["W"][np.triu_indices(100, k=1)])
    assert np.abs(mags - 1e-3).min() > CLEAR * r["max_abs"]  # no entry at the threshold
    assert 0 < r["nnz"] < 4950 and mon.history[-1]["nnz_interactions"] == r["nnz"]
    plain = Monitor()
    est = _notebook_fm(max_iter=2, n_calls=1, callback=plain)
    with _quiet():
        est.fit(z["X"], z["y"])
    assert "nnz_interactions" not in plain.history[0]


def test_all_subsets_regressor():
    from sparsepoly_amd import SparseAllSubsetsRegressor

    X, y = _problem(1000, 80, 6, 4)
    est = SparseAllSubsetsRegressor(n_components=4, solver="pcd", regularizer="omegati", beta=1.0,
                                    gamma=1e-2, max_iter=5, tol=-1, random_state=0,
                                    precision="f64")
    with _quiet():
        est.fit(X, y)
    r = restate(est.P_, est.lams_, top=10)
    st = est.interaction_stats()
    assert (st["nnz"], st["active_features"]) == (r["nnz"], r["active_features"])
    rows, cols, vals = est.top_interactions(10)
    np.testing.assert_array_equal(rows, r["top_rows"])
    np.testing.assert_array_equal(cols, r["top_cols"])
    W = est.interactions()
    np.testing.assert_array_equal(W.row, r["rows"])
    np.testing.assert_array_equal(W.col, r["cols"])


def test_degree3_explicit_lower_block():
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y = _problem(1000, 80, 6, 4)
    est = SparseFactorizationMachineRegressor(degree=3, n_components=4, solver="pcd",
                                              regularizer="omegati", beta=10.0, gamma=1e-3,
                                              max_iter=3, tol=-1, random_state=0, precision="f64")
    with _quiet():
        est.fit(X, y)
    r = restate(est.P_[1], est.lams_, wide=True)  # order degree - 2 holds the degree-2 block
    st = est.interaction_stats()
    assert (st["nnz"], st["active_features"]) == (r["nnz"], r["active_features"])
    _check_stats(st, r, 4, "degree 3, explicit lower block")


# ------------------------------------------------------------------ 9. block and values
@pytest.mark.parametrize("layout", ["P", "Pt"])
def test_block_and_values(layout):
    import ctypes as C

    from sparsepoly_amd import _capi

    P0, lams = _block(21, 31, 300, 0.5)
    P = _live_block(P0, lams, layout)
    k = P.shape[0]
    r = restate(P, lams, wide=True)
    W = r["W"].copy()
    np.fill_diagonal(W, 0.0)
    eng = _engine(P0, lams, layout)
    rng = np.random.RandomState(0)
    J = rng.randint(0, 300, size=40)
    J[5] = J[6]  # repeated indices
    J2 = np.concatenate([J[:10], rng.randint(0, 300, size=25)])  # J[a] == J2[b] happens
    got = eng.interaction_block(0, J, J2)
    want = W[np.ix_(J, J2)]
    assert got.shape == (40, 35)
    assert (np.abs(got.astype(np.longdouble) - want) <= (k + 2) * U * r["bound"][np.ix_(J, J2)]).all()
    assert (got[J[:, None] == J2[None, :]] == 0.0).all()
    assert np.array_equal(eng.interaction_block(0, J), eng.interaction_block(0, J, J))
    rows, cols = rng.randint(0, 300, size=500), rng.randint(0, 300, size=500)
    rows[:7] = cols[:7]
    vals = eng.interaction_values(0, rows, cols)
    assert (np.abs(vals.astype(np.longdouble) - W[rows, cols]) <=
            (k + 2) * U * r["bound"][rows, cols]).all()
    assert (vals[:7] == 0.0).all()
    assert np.array_equal(vals, eng.interaction_values(0, cols, rows))  # either order of ids
    # the same arithmetic in both entries
    assert np.array_equal(eng.interaction_block(0, rows[:20], cols[:20]).diagonal(), vals[:20])
    with pytest.raises(ValueError):
        eng.interaction_values(0, [0], [300])
    with pytest.raises(ValueError):
        eng.interaction_block(0, [-1], [0])
    # byte budget: 12000 x 12000 doubles > 1 GiB, refused before anything is allocated or written
    big = np.zeros(12000, dtype=np.int32)
    out = np.zeros(1)
    rc = eng._lib.spfm_interaction_block(eng._h, 0, 12000, big.ctypes.data_as(_capi._ip), 12000,
                                         big.ctypes.data_as(_capi._ip),
                                         out.ctypes.data_as(_capi._dp))
    assert rc == _capi.SPFM_ERR_INVALID
    assert "budget" in eng._lib.spfm_last_error(eng._h).decode()
    with pytest.raises(ValueError, match="budget"):
        eng.interaction_block(0, big, big)
    eng.close()


def test_errors():
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f32")
    with pytest.raises(ValueError, match="no parameters"):
        eng.interaction_stats(0)
    eng.set_params(np.ones((1, 2, 5)), np.zeros(5), np.ones(2))
    with pytest.raises(ValueError, match="order index"):
        eng.interaction_stats(1)
    with pytest.raises(ValueError, match="tol"):
        eng.interaction_stats(0, -1.0)
    with pytest.raises(ValueError, match="tol"):
        eng.interaction_stats(0, float("nan"))
    assert eng.interaction_stats(0)["nnz"] == 10  # parameters only: no data, no configuration
    assert len(eng.interaction_topk(0, 0)[0]) == 0
    eng.close()
