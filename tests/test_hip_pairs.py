"""``spfm_explain_pairs_*`` and what ``sparsepoly_amd.explain`` builds on them, on the device.
Needs a real MI355X: ``pytest -m gpu``.

Values are compared with the NumPy restatement ``restate_pair_contributions(..., wide=True)``
(``tests/test_pairs_host.py`` holds it equal to brute-force Shapley-Taylor indices).  The bound
comes from the arithmetic of ``pairs_block_kernel`` (``csrc/spfm_pairs.hip.h``) and from no device
run.  A computed pair value is a sum of signed terms
``x_a x_b p_a p_b lams c_st / (t (t - 1) / 2) (-z_b)^r2 (-z_a)^r1 m``, ``m`` a monomial of
``a_v``, ``v + r1 + r2 = t - 2`` (both downdates add terms that cancel in exact arithmetic, so they
are counted with their magnitudes).  Such a term goes through at most

    N = n_i + 6 M + min(k, 64) + n_blocks ceil(k / 64)

roundings (``n_i`` the row's stored entries, ``M`` the degree):
  * inside ``a_v``: one per factor ``p x``, one per multiplication by it, one per addition of the
    recurrence, of which a row has ``n_i``: ``n_i + 2 v``;
  * the first downdate: the subtraction that takes ``a_v`` in, then per step the factor ``z_a``,
    the product and the subtraction: ``1 + 3 r1``; the second: the subtraction that takes ``g`` in,
    then per step ``z_b``, the product, the subtraction: ``1 + 3 r2``; with the line above at most
    ``n_i + 2 + 3 (M - 2) = n_i + 3 M - 4``;
  * ``c / (t (t - 1) / 2)`` (one division by an integer), the product with ``lams``, the product
    with ``h`` and the ``M - 2`` additions of the sum over ``t``: ``M + 1``;
  * ``p_a p_b``, its product with the inner sum, the sum over the components of a chunk
    (``min(k, 64)`` additions), ``x_a x_b`` and the product with it: ``min(k, 64) + 4``;
  * one addition into the pair per chunk of 64 components and block: ``n_blocks ceil(k / 64)``;
  * ``fit_lower='augment'``: ``c_st`` is the host's sum of products of at most ``M - 1`` dummy
    parameters, ``2 (M - 1)`` roundings;
in all ``n_i + 6 M - 1 + min(k, 64) + n_blocks ceil(k / 64)``, rounded up to ``N``.  So
``|device - exact| <= (N + 2) 2^-53 S_hat`` per pair, ``S_hat`` the sum of the magnitudes of the
pair's terms (``pair_majorant`` of ``tests/test_pairs_host.py``, in ``longdouble``); the 2 covers
the second-order terms and the ``longdouble`` reference.  The hessian drops ``x_a x_b`` and the
division: the same ``N`` holds.  ``main`` (``pairs_main_kernel``): ``w x``, then per block
``lams c``, ``p x``, their product, ``k`` additions, one addition into the entry, and the
``2 (M - 1)`` of the host's ``c_s1``: ``N_main = k + 2 M + 2 + 2 n_blocks``.  A table cell or a
group's main adds its ``m`` values in one lane: ``m`` more roundings for each of them.  Each case
prints its largest error as a fraction of its bound before asserting.

Orders are exact.  Where the device order is compared with NumPy's, the NumPy side first asserts,
before the device is touched, that the top K + 1 magnitudes of every row are at least
``CLEAR * max|phi|`` apart; the seeds pass that on the CPU and no case is skipped.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from test_explain_host import COMBOS, majorant, model_output, rows_matrix
from test_pairs_host import numpy_groups, pair_majorant
from test_ranking_host import abs_model, fm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLEAR = 1e-9
# 11 and 12 entries: 55 and 66 pairs, either side of a sweep of 64; empty first and last row
LENGTHS = [0, 1, 2, 3, 11, 12, 63, 64, 65, 130, 0]
D = 400
SMALL = [0, 1, 2, 3, 5, 9, 0]


def _spec(est):
    degree, _, lower = est._obj_pred_args()
    return degree, est.lams_.shape[0], 2 if lower else 1


def _pair_roundings(est, Xc, ptr):
    """N per pair"""
    degree, k, nb = _spec(est)
    n_i = np.repeat(np.diff(Xc.indptr), np.diff(ptr))
    return n_i + 6 * degree + min(k, 64) + nb * -(-k // 64)


def _main_roundings(est):
    degree, k, nb = _spec(est)
    return k + 2 * degree + 2 + 2 * nb


@functools.lru_cache(maxsize=None)
def _case(degree, k, d, fl, lin, seed, lengths, f32=False, cls=None):
    """(est, X) and per mode (Xc, ptr, ca, cb, exact values, exact main, base, bound per pair,
    bound per entry): all NumPy, computed once and shared, never changed"""
    from sparsepoly_amd.explain import restate_pair_contributions

    est = fm(degree, k, d, fl, lin, seed=seed, cls=cls)
    if f32:
        est.precision = "f32"
    X = rows_matrix(list(lengths), d, seed=seed, f32=f32)
    ref = {}
    for mode in ("interaction", "hessian"):
        Xc, ptr, ca, cb, vals, main, base = restate_pair_contributions(est, X, mode, wide=True)
        S, Sm, base_abs = pair_majorant(est, X, mode)
        bound = (_pair_roundings(est, Xc, ptr) + 2) * U * S
        bmain = (_main_roundings(est) + 2) * U * Sm
        for arr in (vals, main, bound, bmain):
            arr.setflags(write=False)
        ref[mode] = (Xc, ptr, ca, cb, vals, main, base, bound, bmain)
    return est, X, ref


def _check_values(got, want, bound, what):
    assert want.dtype == np.longdouble and got.shape == want.shape
    err = np.abs(got.astype(np.longdouble) - want)
    ok = bound > 0
    frac = float((err[ok] / bound[ok]).max(initial=0.0))
    print("%s: largest error %.3g of its bound" % (what, frac))
    assert (err <= bound).all(), (what, frac)


def _double_base(est, X):
    """the base value as the estimator forms it: the host's arithmetic, in double"""
    from sparsepoly_amd.explain import _model

    return float(_model(est, X)[7])


def _check_estimator(est, X, ref, what):
    Xc, ptr, ca, cb, vals, main, base, bound, bmain = ref["interaction"]
    gp, ga, gb, gv, gm, gbase = est.pair_contributions(X, return_main=True, return_base=True)
    assert gv.dtype == np.float64 and gp.dtype == np.int64 and ga.dtype == np.int32
    assert (gp == ptr).all() and (ga == ca).all() and (gb == cb).all()
    assert sp.isspmatrix_csr(gm) and gm.shape == Xc.shape
    assert (gm.indptr == Xc.indptr).all() and (gm.indices == Xc.indices).all()
    assert gbase == _double_base(est, X)
    _check_values(gv, vals, bound, "%s interaction" % what)
    _check_values(gm.data, main, bmain, "%s main" % what)
    Xc, ptr, ca, cb, vals, main, base, bound, bmain = ref["hessian"]
    hp, ha, hb, hv = est.pair_contributions(X, mode="hessian")
    assert (hp == ptr).all() and (ha == ca).all() and (hb == cb).all()
    _check_values(hv, vals, bound, "%s hessian" % what)
    return gv, gm


# ---------------------------------------------------------------- 1. values, main, hessian
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
    est, X, ref = _case(degree, 5, 12, fl, lin, 30 + degree, tuple(SMALL), cls=cls)
    _check_estimator(est, X, ref, "small")


@pytest.mark.parametrize("k,degree,fl", [(k, dg, None) for k in (1, 30, 64, 65, 130)
                                         for dg in (2, 3)]
                         + [(30, 4, None), (30, 5, None), (30, 6, None), (65, 3, "explicit"),
                            (30, 6, "augment")])
def test_shapes_components_and_row_lengths(k, degree, fl):
    """component counts around the chunk of 64; rows of 55 and 66 pairs, either side of a sweep,
    and of 63, 64, 65 and 130 entries; the two-block model and the coefficient table at length"""
    est, X, ref = _case(degree, k, D, fl, True, 40 + k + degree, tuple(LENGTHS))
    _check_estimator(est, X, ref, "k=%d" % k)


def test_a_row_of_300_entries():
    """44 850 pairs: 701 sweeps of one wave"""
    est, X, ref = _case(3, 30, D, None, True, 11, (0, 300, 2))
    _check_estimator(est, X, ref, "300 entries")


@pytest.mark.parametrize("k,degree", [(64, 6), (65, 4)])
def test_every_wave_of_a_workgroup_fills_its_table(k, degree):
    """four consecutive rows of at least 64 entries, k >= 64: the four waves of the first
    workgroup write all 64 columns of their LDS tables at once"""
    est, X, ref = _case(degree, k, D, None, True, 12 + k, (64, 70, 65, 66, 3))
    _check_estimator(est, X, ref, "full waves k=%d" % k)


def test_f32_storage_sees_the_same_inputs():
    """precision='f32': x is rounded to float32 first, so both sides see the same inputs; the
    arithmetic is f64 for either storage type and the bound is unchanged"""
    est, X, ref = _case(3, 30, D, "explicit", True, 6, tuple(LENGTHS), f32=True)
    _check_estimator(est, X, ref, "f32")


# ---------------------------------------------------------------- 2. the three identities
def _explain_bound(est, X):
    """the bound of tests/test_hip_explain.py for the device's feature_contributions"""
    degree, k, nb = _spec(est)
    S1, base_abs = majorant(est, X, "attribution")
    n_i = np.diff(sp.csr_matrix(X).indptr)
    N = np.repeat(n_i, n_i) + 6 * degree + min(k, 64) + nb * -(-k // 64)
    return (N + 2) * U * S1, S1, base_abs


@pytest.mark.parametrize("degree,fl,lin", [(2, None, True), (3, "explicit", True),
                                           (4, "augment", True), (5, "augment", False),
                                           (6, None, False)])
def test_identities_against_predict_and_feature_contributions(degree, fl, lin):
    """(1) sum main + sum phi + base against the existing predict kernel, (2) main + half the
    pairs of an entry against the device's own feature_contributions, each within the sum of the
    two derived bounds; the host adds in longdouble.  predict: a monomial of a_M passes
    n_i' + 2 M roundings (n_i' counts the dummy columns), then ceil(k / 64) lane additions, the
    butterfly's 6, one addition per block; the linear term one product and n_i' + 1 additions."""
    est, X, ref = _case(degree, 65, D, fl, lin, 50 + degree, tuple(LENGTHS))
    Xc, ptr, ca, cb, vals, main, base, bound, bmain = ref["interaction"]
    ld = np.longdouble
    n, n_i = Xc.shape[0], np.diff(Xc.indptr)
    gp, ga, gb, gv, gm = est.pair_contributions(X, return_main=True)
    prow = np.repeat(np.arange(n), np.diff(ptr))
    erow = np.repeat(np.arange(n), n_i)
    total = np.zeros(n, dtype=ld)
    np.add.at(total, prow, gv.astype(ld))
    np.add.at(total, erow, gm.data.astype(ld))
    b1 = np.bincount(prow, weights=bound.astype(np.double), minlength=n) + \
        np.bincount(erow, weights=bmain.astype(np.double), minlength=n)
    n_dummy = est.P_.shape[2] - D
    N_pred = n_i + n_dummy + 2 * degree + 2 + 6 + _spec(est)[2] + 2
    S_abs = model_output(abs_model(est), np.abs(X.toarray()))
    b1 = b1 + (N_pred + 2) * U * S_abs
    err = np.abs(total + base - est.predict(X))
    ok = b1 > 0
    print("efficiency: largest error %.3g of its bound" % float((err[ok] / b1[ok]).max()))
    assert (err <= b1).all()
    assert total[0] == 0 and total[-1] == 0
    # (2)
    fc = est.feature_contributions(X)
    b2, _, _ = _explain_bound(est, X)
    half = gm.data.astype(ld)
    b2 = b2.astype(np.double) + bmain.astype(np.double)
    for i in range(n):
        lo = Xc.indptr[i]
        if n_i[i] > 1:
            ia, ib = np.triu_indices(n_i[i], 1)
            for side in (ia, ib):
                np.add.at(half, lo + side, gv[ptr[i]:ptr[i + 1]].astype(ld) / 2)
                np.add.at(b2, lo + side, bound[ptr[i]:ptr[i + 1]].astype(np.double) / 2)
    err = np.abs(half - fc.data)
    print("consistency: largest error %.3g of its bound" % float((err / b2).max()))
    assert (err <= b2).all()


def test_a_plain_degree_2_model_against_interactions():
    """(3) phi_iab = x_ia x_ib W[a, b] with the W of est.interactions: W[a, b] is a sum of k
    products p p lams (k + 2 roundings), times x x two more; within that plus the pair's bound"""
    est, X, ref = _case(2, 30, D, None, True, 13, tuple(LENGTHS))
    Xc, ptr, ca, cb, vals, main, base, bound, bmain = ref["interaction"]
    W = est.interactions().tocsr()
    gp, ga, gb, gv = est.pair_contributions(X)
    rows = np.repeat(np.arange(Xc.shape[0]), np.diff(ptr))
    Xd = X.toarray()
    Wab = np.asarray(W[ga, gb]).ravel()
    want = Xd[rows, ga] * Xd[rows, gb] * Wab
    S = bound / ((_pair_roundings(est, Xc, ptr) + 2) * U)
    tol = bound.astype(np.double) + (30 + 6) * U * S.astype(np.double)
    err = np.abs(gv - want)
    print("degree 2: largest error %.3g of its bound" % float((err / tol).max()))
    assert np.abs(want).max() > 0 and (err <= tol).all()


# ---------------------------------------------------------------- 3. partition independence
def _slabs(lengths, slab_nnz):
    """the partition rule restated: at most slab_nnz entries and 2 slab_nnz pairs, one row at least"""
    n_i = np.array(lengths)
    pairs = n_i * (n_i - 1) // 2
    count, r0 = 0, 0
    while r0 < len(n_i):
        r1 = r0 + 1
        while r1 < len(n_i) and n_i[r0:r1 + 1].sum() <= slab_nnz and \
                pairs[r0:r1 + 1].sum() <= 2 * slab_nnz:
            r1 += 1
        count, r0 = count + 1, r1
    return count


def test_one_set_of_bits_under_every_partition():
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.explain import _model

    est, X, ref = _case(3, 65, D, "explicit", True, 7, tuple(LENGTHS))
    Xc, blocks, coef, P, w, lams, lin, base = _model(est, X)
    groups = (np.arange(D) % 5).astype(np.int32)
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(P, w, lams)
        got = {}
        # 1000 (2000 pairs): rows 0-5 (29 entries, 125 pairs) stop at the 63-entry row's 1953
        #   pairs; the rows of 64, 65 and 130 entries (2016, 2080, 8385 pairs) exceed the pair
        #   budget on their own and get a slab each, so does the empty last row (the slab before
        #   it is over the pair budget already): 6
        # 100 (200 pairs): rows 0-5, then one row each: 6
        # 1: the empty first row shares the second row's slab, every other row has its own
        for slab, n_slabs in ((0, 1), (1000, 6), (100, 6), (1, len(LENGTHS) - 1)):
            assert _slabs(LENGTHS, slab or 1 << 23) == n_slabs
            eng.explain_set_partition(slab)
            ptr, vals, mn = eng.explain_pairs(Xc, blocks, coef, lin, main=True)
            info = eng.explain_info()
            assert info["slabs"] == n_slabs and info["slab_nnz"] == slab, info
            _, hess, _ = eng.explain_pairs(Xc, blocks, coef, lin, "hessian")
            ca, cb, tv = eng.explain_pairs_topk(Xc, blocks, coef, lin, 7)
            assert eng.explain_info()["slabs"] == n_slabs
            cells, gm = eng.explain_pairs_grouped(Xc, blocks, coef, lin, 5, groups)
            assert eng.explain_info()["slabs"] == n_slabs
            got[slab] = (vals, mn, hess, ca, cb, tv, cells, gm)
        assert eng.explain_info()["scratch_kib"] > 0
    finally:
        eng.close()
    n_i = np.array(LENGTHS)
    assert got[0][0].shape == ((n_i * (n_i - 1) // 2).sum(),) and np.abs(got[0][0]).min() > 0
    for slab in (1000, 100, 1):
        for a, b in zip(got[0], got[slab]):
            assert a.tobytes() == b.tobytes(), slab


# ---------------------------------------------------------------- 4. top-K
def _numpy_topk(ref, K):
    """NumPy's stable order of the exact values, (|phi| descending, pair index ascending),
    padded; asserts first that the top K + 1 magnitudes of every row are CLEAR * max|phi| apart"""
    Xc, ptr, ca, cb, want = ref[:5]
    n = Xc.shape[0]
    A = np.full((n, K), -1, dtype=np.int32)
    B = np.full((n, K), -1, dtype=np.int32)
    pos = np.full((n, K), -1, dtype=np.int64)
    scale = np.abs(want).max()
    for i in range(n):
        mag = np.abs(want[ptr[i]:ptr[i + 1]])
        order = np.argsort(-mag, kind="stable")
        top = mag[order][:K + 1]
        if top.size > 1:
            assert np.diff(-top).min() > CLEAR * scale, "top K + 1 magnitudes too close"
        m = min(K, mag.size)
        A[i, :m], B[i, :m] = ca[ptr[i] + order[:m]], cb[ptr[i] + order[:m]]
        pos[i, :m] = ptr[i] + order[:m]
    return A, B, pos


@pytest.mark.parametrize("K", [1, 7, 64])
@pytest.mark.parametrize("mode", ["interaction", "hessian"])
def test_top_k_is_numpys_order(K, mode):
    est, X, refs = _case(3, 30, D, "explicit", True, 8, tuple(LENGTHS))
    ref = refs[mode]
    A, B, pos = _numpy_topk(ref, K)
    ga, gb, gv = est.top_pair_contributions(X, K, mode=mode)
    assert ga.dtype == gb.dtype == np.int32 and gv.dtype == np.float64
    assert ga.shape == gb.shape == gv.shape == (len(LENGTHS), K)
    assert (ga == A).all() and (gb == B).all()
    filled = pos >= 0
    assert (gv[~filled] == 0).all() and (ga[~filled] == -1).all() and (gb[~filled] == -1).all()
    _check_values(gv[filled], ref[4][pos[filled]], ref[7][pos[filled]], "top-%d %s" % (K, mode))
    # rows with fewer pairs than K are padded: rows of 0 and 1 entries entirely, the row of 2
    # entries after its one pair, the row of 3 after its three
    assert (ga[0] == -1).all() and (ga[1] == -1).all() and (ga[-1] == -1).all()
    assert ga[2, 0] >= 0 and (ga[2, 1:] == -1).all()
    if K > 3:
        assert (ga[3, :3] >= 0).all() and (ga[3, 3:] == -1).all()
    # the listed values are the device's own values of those pairs
    full = est.pair_contributions(X, mode=mode)[3]
    assert (gv[filled] == full[pos[filled]]).all()


def test_top_k_above_the_cap_is_refused():
    est = fm(2, 3, 10)
    X = rows_matrix([2, 3], 10)
    with pytest.raises(ValueError, match="exceeds the cap"):
        est.top_pair_contributions(X, 65)
    ca, cb, vals = est.top_pair_contributions(X, 64)  # the cap itself is served
    assert ca.shape == (2, 64) and (ca[0, 1:] == -1).all() and (ca[1, :3] >= 0).all()


def test_top_k_tie_goes_to_the_lower_pair_index():
    """columns 3 and 9 of P_ and w_ identical, equal x in a row: the pairs (3, c) and (9, c) and
    the pairs (c, 3) and (c, 9) have bit-equal values, the one with the lower pair index first"""
    est = fm(3, 5, 12, "explicit", True, seed=9)
    est.P_[:, :, 9] = est.P_[:, :, 3]
    X = sp.csr_matrix(np.array([[0, 1.5, 0, 0.75, 0, 0, -2.0, 0, 0, 0.75, 0, 0.5],
                                [0.5, 0, 0, -1.25, 0, 0, 0, 0, 0, -1.25, 0, 0]]))
    ptr, ca, cb, vals = est.pair_contributions(X)
    assert list(np.diff(ptr)) == [10, 3]
    value = {(i, a, b): v for i in range(2)
             for a, b, v in zip(ca[ptr[i]:ptr[i + 1]], cb[ptr[i]:ptr[i + 1]],
                                vals[ptr[i]:ptr[i + 1]])}
    ties = [((0, 1, 3), (0, 1, 9)), ((0, 3, 11), (0, 9, 11)), ((1, 0, 3), (1, 0, 9))]
    for first, second in ties:
        assert value[first] == value[second] != 0
    ta, tb, tv = est.top_pair_contributions(X, 10)
    for first, second in ties:
        i = first[0]
        listed = list(zip(ta[i], tb[i]))
        assert listed.index(second[1:]) == listed.index(first[1:]) + 1
        assert tv[i, listed.index(first[1:])] == value[first]
    assert (ta[0] >= 0).all() and list(ta[1, 3:]) == [-1] * 7


# ---------------------------------------------------------------- 5. group tables
@pytest.mark.parametrize("G", [1, 3, 32])
def test_group_tables(G):
    """against the restatement grouped in NumPy; a cell (a group's main) that adds m values in
    one lane passes m more roundings per value.  Group G - 1 holds no stored entry: its column is
    not stored in any row (G > 1)."""
    est, X, refs = _case(4, 30, D, "augment", True, 14, tuple(LENGTHS))
    Xc, ptr, ca, cb, vals, main, base, bound, bmain = refs["interaction"]
    rng = np.random.RandomState(G)
    groups = rng.randint(0, max(G - 1, 1), size=D)
    if G > 1:
        free = np.setdiff1d(np.arange(D), Xc.indices)
        assert free.size > 0
        groups[free[0]] = G - 1
    want_T, want_m = numpy_groups(Xc, ptr, vals, main, groups, G)
    ones_T, ones_m = numpy_groups(Xc, ptr, np.ones(vals.shape), np.ones(main.shape), groups, G)
    S = bound / ((_pair_roundings(est, Xc, ptr) + 2) * U)
    Sm = bmain / ((_main_roundings(est) + 2) * U)
    # sum of (N + 2 + m) U S over a cell: the summed bounds plus m U times the summed majorants
    bT, bm = numpy_groups(Xc, ptr, bound.copy(), bmain.copy(), groups, G)
    eT, em = numpy_groups(Xc, ptr, U * S, U * Sm, groups, G)
    bT, bm = bT + ones_T * eT, bm + ones_m * em
    T, mg, gbase = est.group_contributions(X, groups, return_base=True)
    assert T.shape == (len(LENGTHS), G, G) and mg.shape == (len(LENGTHS), G)
    assert T.dtype == np.float64 and gbase == _double_base(est, X)
    assert (np.tril(T, -1) == 0).all()
    _check_values(T, want_T, bT, "G=%d table" % G)
    _check_values(mg, want_m, bm, "G=%d main" % G)
    assert (T[0] == 0).all() and (T[-1] == 0).all() and (mg[0] == 0).all()
    if G > 1:
        assert (T[:, :, G - 1] == 0).all() and (mg[:, G - 1] == 0).all()
        assert np.count_nonzero(T) > 0


# ---------------------------------------------------------------- 6. errors, through the C ABI
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
    group = _capi.i32(np.arange(10) % 2)
    vals, mn = np.full(4, 7.0), np.full(X.nnz, 7.0)
    ca, cb = np.full((3, 2), 7, dtype=np.int32), np.full((3, 2), 7, dtype=np.int32)
    val = np.full((3, 2), 7.0)
    cells, gmain = np.full((3, 3), 7.0), np.full((3, 2), 7.0)
    dp, ip = _capi._dp, _capi._ip
    eng = HipEngine(0, "f64")
    lib, h = eng._lib, eng._h

    def listing(n=3, ia=ia, ja=ja, order=order, degree=degree, mode=0, main=True):
        return lib.spfm_explain_pairs_csr(h, n, ia[1], ja[1], da[1], 1, order[1], degree[1],
                                          coef[1], 1, mode, vals.ctypes.data_as(dp),
                                          mn.ctypes.data_as(dp) if main else None)

    def topk(K, mode=0):
        return lib.spfm_explain_pairs_topk_csr(h, 3, ia[1], ja[1], da[1], 1, order[1], degree[1],
                                               coef[1], 1, mode, K, ca.ctypes.data_as(ip),
                                               cb.ctypes.data_as(ip), val.ctypes.data_as(dp))

    def grouped(G, group=group):
        return lib.spfm_explain_pairs_grouped_csr(h, 3, ia[1], ja[1], da[1], 1, order[1],
                                                  degree[1], coef[1], 1, G, group[1],
                                                  cells.ctypes.data_as(dp),
                                                  gmain.ctypes.data_as(dp))

    def message():
        return lib.spfm_last_error(h).decode()

    try:
        for call in (listing, lambda: topk(1), lambda: grouped(2)):
            assert call() == _capi.SPFM_ERR_INVALID and "no parameters set" in message()
        eng.set_params(est.P_, est.w_, est.lams_)
        # everything explain_check refuses
        assert listing(degree=_capi.i32(np.array([7]))) == _capi.SPFM_ERR_UNSUPPORTED
        assert "degree outside 2..6" in message()
        assert listing(degree=_capi.i32(np.array([1]))) == _capi.SPFM_ERR_UNSUPPORTED
        assert listing(order=_capi.i32(np.array([1]))) == _capi.SPFM_ERR_INVALID
        assert "order_idx outside the parameters" in message()
        bad = X.indices.copy()
        bad[-1] = 10  # = d
        assert listing(ja=_capi.i32(bad)) == _capi.SPFM_ERR_INVALID
        assert "column index out of range" in message()
        # modes, K, G, group ids
        assert listing(mode=2) == _capi.SPFM_ERR_INVALID and "mode must be" in message()
        assert topk(2, mode=-1) == _capi.SPFM_ERR_INVALID and "mode must be" in message()
        assert listing(mode=1) == _capi.SPFM_ERR_INVALID and "out_main" in message()
        assert topk(0) == _capi.SPFM_ERR_INVALID and "K must be >= 1" in message()
        assert topk(65) == _capi.SPFM_ERR_UNSUPPORTED and "SPFM_PAIRS_MAX_K" in message()
        assert grouped(0) == _capi.SPFM_ERR_INVALID and "G must be >= 1" in message()
        assert grouped(33) == _capi.SPFM_ERR_UNSUPPORTED and "SPFM_PAIRS_MAX_GROUPS" in message()
        assert grouped(1) == _capi.SPFM_ERR_INVALID and "group id out of range" in message()
        assert grouped(2, _capi.i32(np.arange(10) % 2 - 1)) == _capi.SPFM_ERR_INVALID
        # a listing above SPFM_PAIRS_MAX_BYTES (one valid row of 16 500 entries: 1.09 GB of pair
        # values) and a row of more than 65 536 entries
        wide = fm(2, 1, 16500)
        eng.set_params(wide.P_, wide.w_, wide.lams_)
        big_ptr = _capi.i64(np.array([0, 16500]))
        big_idx = _capi.i32(np.arange(16500))
        big_val = _capi.f64(np.ones(16500))
        c1 = np.zeros((1, 1, 7))
        c1[0, :, 2] = 1
        c1 = _capi.f64(c1)
        assert 16500 * 16499 // 2 * 8 > _capi.PAIRS_MAX_BYTES
        rc = lib.spfm_explain_pairs_csr(h, 1, big_ptr[1], big_idx[1], big_val[1], 1, order[1],
                                        degree[1], c1[1], 1, 0, vals.ctypes.data_as(dp), None)
        assert rc == _capi.SPFM_ERR_UNSUPPORTED and "SPFM_PAIRS_MAX_BYTES" in message()
        wide = fm(2, 1, 65537)
        eng.set_params(wide.P_, wide.w_, wide.lams_)
        big_ptr = _capi.i64(np.array([0, 2, 65539]))
        big_idx = _capi.i32(np.concatenate([[0, 1], np.arange(65537)]))
        big_val = _capi.f64(np.ones(65539))
        rc = lib.spfm_explain_pairs_topk_csr(h, 2, big_ptr[1], big_idx[1], big_val[1], 1, order[1],
                                             degree[1], c1[1], 1, 0, 2, ca.ctypes.data_as(ip),
                                             cb.ctypes.data_as(ip), val.ctypes.data_as(dp))
        assert rc == _capi.SPFM_ERR_UNSUPPORTED and "more than 65536" in message()
        eng.set_params(est.P_, est.w_, est.lams_)
        # nothing was written by any refused call, nor by n = 0
        assert listing(n=0) == _capi.SPFM_OK
        for arr in (vals, mn, ca, cb, val, cells, gmain):
            assert (arr == 7).all()
        # ... and the handle is usable
        assert listing() == _capi.SPFM_OK and topk(2) == _capi.SPFM_OK
        assert grouped(2) == _capi.SPFM_OK
        assert (vals != 7).all() and (mn != 7).all()
        assert list(ca[1]) == [-1, -1] and list(cb[1]) == [-1, -1] and list(val[1]) == [0, 0]
        assert ca[0, 0] == X.indices[0] and cb[0, 0] == X.indices[1] and ca[0, 1] == -1
        assert val[0, 0] == vals[0]
        assert (cells[1] == 0).all() and (gmain[1] == 0).all() and (cells != 7).all()
        assert listing(mode=1, main=False) == _capi.SPFM_OK
        with pytest.raises(ValueError, match="mode must be"):
            eng.explain_pairs(X, [(0, 2)], coef[0], True, "shap")
        with pytest.raises(ValueError, match="one id per feature"):
            eng.explain_pairs_grouped(X, [(0, 2)], coef[0], True, 2, np.zeros(9))
        assert eng.explain_info()["scratch_kib"] > 0
        eng.set_params(est.P_, est.w_, est.lams_)  # new parameters: the scratch is gone
        assert eng.explain_info()["scratch_kib"] == 0
    finally:
        eng.close()
