"""``spfm_bank_group_curve``, ``ModelBank.group_curve``, ``cross_validate_path`` with the curve
metrics, ``average_precision`` and ``operating_point`` on the device.  Needs a real MI355X:
``pytest -m gpu``.

The yardstick is ``restate_group_curve`` (NumPy; held to a loop over the runs in ``Fraction`` and
to scikit-learn in ``tests/test_bank_curve_host.py``) applied to the scores of the bank's own
``decision_function``: what is under test is the top-down walk, not the scoring pass or the sorts.

Shapes: ``B = SPFM_BANK_RANK_BLOCK`` sorted positions per workgroup of the walk, ``n = 3 B + 37``
rows (four workgroups, the last one short), 12 columns, and the three members of
``tests/test_hip_bank_auc.py``: every parameter zero (one run over all four blocks), about 40 runs
(open across every block boundary), n distinct scores.  These are the smallest shapes at which a
carry, a run open at a block start and a short last block can go wrong.

Unweighted, counts, thresholds, ``best_f1`` and ``ks`` are functions of the scores and labels
alone: equal or wrong.  ``average_precision`` is a sum of doubles whose order differs between the
device (blocks of B positions) and the restatement (one after the other): both are within
``(2 n + 8) u`` relative of the exact value (``tests/test_bank_curve_host.py``), so they are within
``(4 n + 16) u``, u = 2^-53, of each other -- the bound asserted here.  For the same reason the
average precision of integer weights and that of physically replicated rows (another n, so other
blocks) are held to that bound and not to equality; every other field of the two is equal.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
from test_ranking_host import fm

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
D = 12
FIELDS = ("average_precision", "pos_weight", "neg_weight", "best_f1", "f1_threshold", "f1_tp",
          "f1_fp", "ks", "ks_threshold", "ks_tp", "ks_fp")
EXACT = tuple(k for k in FIELDS if k != "average_precision") + ("counts",)


def _B():
    from sparsepoly_amd import _capi

    return _capi.BANK_RANK_BLOCK


def _tied_rows(n, seed=3):
    """about 40 distinct rows over the columns 0..10, each repeated, in shuffled order; column 11
    holds a value of its own in every row"""
    rng = np.random.RandomState(seed)
    base = np.where(rng.rand(40, D) < 0.4, rng.randn(40, D), 0.0)
    base[0] = 0.0
    V = base[rng.randint(0, 40, size=n)]
    V[:, D - 1] = rng.permutation(n) + 1.0
    return sp.csr_matrix(V)


def _members():
    """zero: every parameter 0 (one score); tied: blind to column 11 (identical rows give
    bit-identical scores); distinct: a linear weight on column 11 as well"""
    zero, tied, distinct = (fm(2, k, D, None, True, seed=40 + k) for k in (2, 3, 5))
    zero.P_[:] = 0.0
    zero.w_[:] = 0.0
    for e in (tied, distinct):
        e.P_[:, :, D - 1] = 0.0
        e.w_[D - 1] = 0.0
    distinct.w_[D - 1] = 1e-3
    return [zero, tied, distinct]


def _host_sets():
    """the host case's kinds of sets over 5 groups: one group, a union, one without positives
    (group 2, see the fixture), an empty one (group 4 holds no row), a complement per member"""
    sets = np.zeros((3, 5, 5), dtype=bool)
    sets[:, 0, 0] = True
    sets[:, 1, [0, 1]] = True
    sets[:, 2, 2] = True
    sets[:, 3, 4] = True
    for f in range(3):
        sets[f, 4] = np.arange(5) != f
    return sets


@pytest.fixture(scope="module")
def case():
    from sparsepoly_amd import ModelBank

    n = 3 * _B() + 37
    X = _tied_rows(n)
    ests = _members()
    rng = np.random.RandomState(8)
    y = np.where(rng.rand(n) < 0.3, 1.0, -1.0)
    Y = np.where(rng.rand(n, 3) < 0.5, 1.0, -1.0)
    g = rng.randint(0, 4, size=n).astype(np.int32)  # group 4 holds no row
    y[g == 2] = -1.0                                  # group 2 holds no positive
    Y[g == 2] = -1.0
    with ModelBank(ests) as bank:
        scores = bank.decision_function(X)
        assert len(np.unique(scores[:, 0] + 0.0)) == 1
        runs = np.unique(scores[:, 1], return_counts=True)[1]
        assert len(runs) <= 45 and runs.max() > 10
        assert len(np.unique(scores[:, 2])) == n
        yield bank, ests, X, scores, y, Y, g


def _same(got, want, keys=FIELDS + ("counts", "auc", "pairs")):
    for k in keys:
        assert (k in got) == (k in want), k
        if k in got:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            assert np.array_equal(got[k], want[k], equal_nan=True), k


def _ap_close(got, want, n, what):
    """``average_precision`` within (4 n + 16) u relative; prints the largest share of the bound"""
    a, b = got["average_precision"], np.asarray(want["average_precision"], dtype=np.double)
    assert a.shape == b.shape and (np.isnan(a) == np.isnan(b)).all(), what
    ok = ~np.isnan(b)
    tol = (4 * n + 16) * U53
    err = np.abs(a[ok] - b[ok])
    share = float((err / (tol * b[ok])).max()) if ok.any() else 0.0
    print("%s: average precision, largest error %.3g of its bound%s"
          % (what, share, "" if share else " (the same bits)"))
    assert (err <= tol * b[ok]).all(), what


def _unweighted(got, want, n, what):
    _same(got, want, EXACT)
    _ap_close(got, want, n, what)


# ---------------------------------------------------------------- 1. unweighted
def test_unweighted_one_set_and_groups(case):
    from sparsepoly_amd.bank import restate_group_curve

    bank, ests, X, scores, y, Y, g = case
    n = X.shape[0]
    got = bank.group_curve(X, y)
    want = restate_group_curve(scores, y, None, None, 1, None)
    assert set(got) == set(FIELDS) | {"counts"}
    assert got["counts"].shape == (3, 1, 6) and got["counts"].dtype == np.int64
    _unweighted(got, want, n, "one set")
    npos, nneg = int((y > 0).sum()), int((y <= 0).sum())
    assert (got["counts"][:, 0, :2] == [npos, nneg]).all()
    # one run over all rows: one candidate
    assert got["counts"][0, 0].tolist() == [npos, nneg, npos, nneg, npos, nneg]
    assert got["average_precision"][0, 0] == float(npos) * (float(npos) / float(n)) / float(npos)
    assert got["ks"][0, 0] == 0.0
    assert got["f1_threshold"][0, 0] == 0.0 and not np.signbit(got["f1_threshold"][0, 0])
    sets = _host_sets()
    for t, what in ((y, "shared y"), (Y, "per-member Y")):
        got = bank.group_curve(X, t, groups=g, n_groups=5, sets=sets)
        _unweighted(got, restate_group_curve(scores, t, None, g, 5, sets), n, "5 groups, " + what)
        assert np.isnan(got["average_precision"][:, 2:4]).all()
        assert (got["counts"][:, 2, 0] == 0).all() and (got["counts"][:, 2, 1] > 0).all()
        assert (got["counts"][:, 3] == 0).all()
    default = bank.group_curve(X, y, groups=g, n_groups=5)  # sets=None: one set per group
    _unweighted(default, restate_group_curve(scores, y, None, g, 5, None), n, "one set per group")


# ---------------------------------------------------------------- 2. where the maximum sits
def _labels_down_to(scores_f, q_last):
    """+1 for the rows at the top-down positions 0 .. q_last of one member, -1 below; whole runs"""
    order = np.argsort(-scores_f, kind="stable")
    cut = scores_f[order[q_last]]
    return np.where(scores_f >= cut, 1.0, -1.0), cut


def test_the_maximum_in_each_place(case):
    from sparsepoly_amd.bank import restate_group_curve

    bank, ests, X, scores, y, Y, g = case
    n, B = X.shape[0], _B()
    rng = np.random.RandomState(21)
    tied, distinct = scores[:, 1], scores[:, 2]
    down = -np.sort(-tied)
    # a run of the tied member that straddles the boundary between the first two blocks
    assert down[B - 1] == down[B]
    first, last = np.flatnonzero(down == down[B])[[0, -1]]
    assert first < B <= last
    places = {
        "the first run of the first block": (0, 0),
        "a run that straddles a block boundary": (B, B),
        "a run in the short last block": (3 * B + 5, 3 * B + 5),
    }
    for what, (q_tied, q_distinct) in places.items():
        Yp = np.where(rng.rand(n, 3) < 0.5, 1.0, -1.0)
        Yp[:, 1], cut_tied = _labels_down_to(tied, q_tied)
        Yp[:, 2], cut_distinct = _labels_down_to(distinct, q_distinct)
        want = restate_group_curve(scores, Yp, None, None, 1, None)
        # where it was meant to be: F1 = 1 exactly there, and nowhere else
        assert want["f1_threshold"][1, 0] == cut_tied and want["best_f1"][1, 0] == 1.0, what
        assert want["f1_threshold"][2, 0] == cut_distinct and want["best_f1"][2, 0] == 1.0, what
        assert want["counts"][2, 0, 2] == q_distinct + 1 and want["counts"][2, 0, 3] == 0
        assert want["ks"][1, 0] == 1.0 and want["ks_threshold"][2, 0] == cut_distinct
        _unweighted(bank.group_curve(X, Yp), want, n, what)
    # the straddling run again with noise below it, so that the maximum is no longer 1
    Yp[:, 1] = np.where((tied < down[B]) & (rng.rand(n) < 0.2), 1.0, _labels_down_to(tied, B)[0])
    want = restate_group_curve(scores, Yp, None, None, 1, None)
    assert want["f1_threshold"][1, 0] == down[B] and want["best_f1"][1, 0] < 1.0
    _unweighted(bank.group_curve(X, Yp), want, n, "a straddling run under noise")


# ---------------------------------------------------------------- 3. ties between maxima
def test_ties_between_maxima_report_the_higher_score(case):
    from sparsepoly_amd.bank import restate_group_curve

    bank, ests, X, scores, y, Y, g = case
    n, B = X.shape[0], _B()
    order = np.argsort(-scores[:, 2], kind="stable")  # the distinct member, from the top
    Yt = np.tile(y[:, None], (1, 3))

    def labels(a, P):
        # a positives on top, P (P - a) / a negatives, P - a positives, negatives: F1 is
        # 2 a / (a + P) at the first stretch's end and 2 P / (2 P + P (P - a) / a), the same
        # number, at the third's; lower everywhere else
        x = P * (P - a) // a
        t = -np.ones(n)
        t[order[:a]] = 1.0
        t[order[a + x:a + x + (P - a)]] = 1.0
        return t, scores[order[a - 1], 2], scores[order[a + x + (P - a) - 1], 2]

    # inside the first block, and across blocks: the second maximum ends in the second block
    for a, P, what in ((1, 2, "inside a block"), (100, 200, "across blocks")):
        Yt[:, 2], high, low = labels(a, P)
        assert what != "across blocks" or a - 1 < B <= a + P * (P - a) // a + (P - a) - 1 < 2 * B
        want = restate_group_curve(scores, Yt, None, None, 1, None)
        tp, fp = P, P * (P - a) // a
        assert 2 * a * (tp + fp + P) == 2 * tp * (a + P)          # an equality of integers
        assert want["f1_threshold"][2, 0] == high > low
        assert want["counts"][2, 0, 2:4].tolist() == [a, 0]
        got = bank.group_curve(X, Yt)
        _unweighted(got, want, n, "tie " + what)
        assert got["f1_threshold"][2, 0] == high
        # the lower one alone wins when the upper one is spoilt by one negative above it
        Yt[order[0], 2] = -1.0
        want = restate_group_curve(scores, Yt, None, None, 1, None)
        assert want["f1_threshold"][2, 0] == low
        _unweighted(bank.group_curve(X, Yt), want, n, "tie broken " + what)


# ---------------------------------------------------------------- 4. weighted
def _weighted_close(got, want, n, what):
    """the bounds of tests/test_bank_curve_host.py against a wide restatement"""
    tol = (4 * n + 16) * U53
    worst = 0.0
    for k in FIELDS:
        a, b = got[k], np.asarray(want[k], dtype=np.double)
        assert a.shape == b.shape and (np.isnan(a) == np.isnan(b)).all(), (what, k)
    assert "counts" not in got
    for k in ("f1_threshold", "ks_threshold"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    for k, rel, bound in (("average_precision", True, tol), ("best_f1", True, tol),
                          ("ks", False, tol), ("pos_weight", True, n * U53),
                          ("neg_weight", True, n * U53), ("f1_tp", True, n * U53),
                          ("f1_fp", True, n * U53), ("ks_tp", True, n * U53),
                          ("ks_fp", True, n * U53)):
        a, b = got[k], np.asarray(want[k], dtype=np.double)
        ok = ~np.isnan(b)
        err = np.abs(a[ok] - b[ok])
        lim = bound * np.abs(b[ok]) if rel else np.full(err.shape, bound)
        assert (err <= lim).all(), (what, k)
        nz = lim > 0
        if nz.any():
            worst = max(worst, float((err[nz] / lim[nz]).max()))
    print("%s: largest error %.3g of its bound" % (what, worst))


def test_weighted_against_the_wide_restatement(case):
    from sparsepoly_amd.bank import restate_group_curve

    bank, ests, X, scores, y, Y, g = case
    n = X.shape[0]
    w = np.random.RandomState(4).rand(n) + 0.5
    sets = _host_sets()
    for t, what in ((y, "shared y"), (Y, "per-member Y")):
        got = bank.group_curve(X, t, groups=g, n_groups=5, sample_weight=w, sets=sets)
        want = restate_group_curve(scores, t, w, g, 5, sets, wide=True)
        _weighted_close(got, want, n, "uniform weights, %s" % what)
    w0 = np.random.RandomState(2).randint(0, 4, size=n) * 0.75  # zero weights
    got = bank.group_curve(X, Y, sample_weight=w0)
    _weighted_close(got, restate_group_curve(scores, Y, w0, None, 1, None, wide=True), n,
                    "weights with zeros")


def test_integer_weights_equal_replicated_rows(case):
    bank, ests, X, scores, y, Y, g = case
    n = X.shape[0]
    w = np.random.RandomState(2).randint(0, 4, size=n).astype(np.double)
    assert (w == 0).any()
    rep = np.repeat(np.arange(n), w.astype(int))
    sets = _host_sets()
    got = bank.group_curve(X, Y, groups=g, n_groups=5, sample_weight=w, sets=sets)
    flat = bank.group_curve(X[rep], Y[rep], groups=g[rep], n_groups=5, sets=sets)
    assert "counts" not in got
    _same(got, flat, tuple(k for k in FIELDS if k != "average_precision"))  # thresholds included
    assert (got["f1_tp"] == flat["counts"][:, :, 2]).all()
    assert (got["ks_fp"] == flat["counts"][:, :, 5]).all()
    assert not np.isnan(got["ks"][:, [0, 1, 4]]).any()
    _ap_close(got, flat, len(rep), "integer weights against replicated rows")


# ---------------------------------------------------------------- 5. invariance of bits
def _both(bank, X, Y, w, **kw):
    return bank.group_curve(X, Y, **kw), bank.group_curve(X, Y, sample_weight=w, **kw)


def test_slabs_do_not_change_a_bit(case):
    bank, ests, X, scores, y, Y, g = case
    w = np.random.RandomState(5).rand(X.shape[0]) * 2
    kw = dict(groups=g, n_groups=5, sets=_host_sets(), auc=True)
    one = _both(bank, X, Y, w, **kw)
    again = _both(bank, X, Y, w, **kw)
    parts = []
    try:
        for cut in (4, 9):
            bank.set_partition(X.nnz // cut)
            parts.append(_both(bank, X, Y, w, **kw))
            assert bank.info()["slabs"] >= cut - 1
    finally:
        bank.set_partition(0)
    for other in [again] + parts:
        for a, b in zip(one, other):
            _same(a, b)


def test_batches_of_members_do_not_change_a_bit(case, monkeypatch):
    bank, ests, X, scores, y, Y, g = case
    w = np.random.RandomState(6).rand(X.shape[0]) + 0.5
    held = np.array([3, 0, 2])
    own = held[:, None] == np.arange(5)[None, :]
    kw = dict(groups=g, n_groups=5, sets=np.stack([own, ~own, own | ~own], axis=1), auc=True)
    whole = _both(bank, X, Y, w, **kw)
    for cap in ("1", "2"):
        monkeypatch.setenv("SPFM_BANK_AUC_BATCH", cap)
        for a, b in zip(whole, _both(bank, X, Y, w, **kw)):
            _same(a, b)
    assert len({tuple(c) for c in whole[0]["counts"][:, 2]}) == 3  # the members differ


def test_a_member_first_and_last_in_the_bank(case):
    from sparsepoly_amd import ModelBank

    bank, ests, X, scores, y, Y, g = case
    w = np.random.RandomState(7).rand(X.shape[0]) + 0.25
    sets = _host_sets()
    kw = dict(groups=g, n_groups=5)
    full = _both(bank, X, Y, w, sets=sets, **kw)
    with ModelBank(ests[::-1]) as rev:
        back = _both(rev, X, Y[:, ::-1], w, sets=sets[::-1], **kw)
    with ModelBank([ests[1]]) as solo:
        alone = _both(solo, X, Y[:, 1], w, sets=sets[1], **kw)
    for a, b, c in zip(full, back, alone):
        for k in a:
            assert np.array_equal(a[k], b[k][::-1], equal_nan=True), k   # first <-> last
            assert np.array_equal(a[k][1], c[k][0], equal_nan=True), k


# ---------------------------------------------------------------- 6. the AUC from the same call
def test_auc_from_the_same_pass(case):
    bank, ests, X, scores, y, Y, g = case
    w = np.random.RandomState(9).rand(X.shape[0]) + 0.5
    kw = dict(groups=g, n_groups=5, sets=_host_sets())
    for sw in (None, w):
        plain = bank.group_curve(X, Y, sample_weight=sw, **kw)
        both = bank.group_curve(X, Y, sample_weight=sw, auc=True, **kw)
        auc = bank.group_auc(X, Y, sample_weight=sw, **kw)
        assert "auc" not in plain and "pairs" not in plain
        assert ("pairs" in both) == (sw is None)
        _same(both, auc, ("auc", "pairs"))
        for k in ("pos_weight", "neg_weight"):  # the two walks add the weights from opposite ends
            if sw is None:
                assert np.array_equal(both[k], auc[k]), k
            else:
                assert (np.abs(both[k] - auc[k]) <= 2 * X.shape[0] * U53 * auc[k]).all(), k
        _same(both, plain, FIELDS + ("counts",))
        assert not np.isnan(both["auc"][:, [0, 1, 4]]).any()


# ---------------------------------------------------------------- 7. edges
def test_small_shapes():
    from sparsepoly_amd import ModelBank
    from sparsepoly_amd.bank import restate_group_curve

    B = _B()
    est = fm(2, 3, D, None, True, seed=77)
    X = _tied_rows(B + 1, seed=1)
    y = np.where(np.arange(B + 1) % 3 == 0, 1.0, -1.0)
    g = (np.arange(B + 1) % 2).astype(np.int32)
    yg = np.where(g == 0, 1.0, -1.0)   # group 0: positives only, group 1: negatives only
    with ModelBank([est]) as b:
        s = b.decision_function(X)
        for n in (1, 2, 37, B, B + 1):  # one short block, a full one, a block of one position
            got = b.group_curve(X[:n], y[:n])
            _unweighted(got, restate_group_curve(s[:n], y[:n], None, None, 1, None), n,
                        "n = %d" % n)
            w = np.arange(n) % 3 * 0.5
            gw = b.group_curve(X[:n], y[:n], sample_weight=w)
            _weighted_close(gw, restate_group_curve(s[:n], y[:n], w, None, 1, None, wide=True), n,
                            "n = %d, weighted" % n)
        one = b.group_curve(X[:1], y[:1])                           # n = 1: a positive
        assert one["counts"][0, 0].tolist() == [1, 0, 1, 0, 0, 0]
        assert one["average_precision"][0, 0] == 1.0 and one["best_f1"][0, 0] == 1.0
        assert one["f1_threshold"][0, 0] == s[0, 0] and np.isnan(one["ks"][0, 0])
        # a set of positives only, one without positives, an empty one (group 2)
        got = b.group_curve(X, yg, groups=g, n_groups=3)
        _unweighted(got, restate_group_curve(s, yg, None, g, 3, None), B + 1, "one-class sets")
        assert got["average_precision"][0, 0] == 1.0 and got["best_f1"][0, 0] == 1.0
        assert got["f1_threshold"][0, 0] == s[g == 0, 0].min() and np.isnan(got["ks"][0, 0])
        assert np.isnan(got["ks_threshold"][0, 0]) and got["ks_tp"][0, 0] == 0
        for u in (1, 2):
            for k in ("average_precision", "best_f1", "f1_threshold", "ks", "ks_threshold"):
                assert np.isnan(got[k][0, u]), (u, k)
        assert got["counts"][0].tolist() == [[(B + 2) // 2, 0, (B + 2) // 2, 0, 0, 0],
                                             [0, (B + 1) // 2, 0, 0, 0, 0], [0] * 6]
    # n = 0: through the C entry (test_entry_point_refusals); the estimators' checks want a row


# ---------------------------------------------------------------- 8. the C entry point
def test_entry_point_refusals(monkeypatch):
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    lib = eng._lib
    d, F, k, n = 6, 2, 3, 3
    lengths = [2, 0, 3]
    rng = np.random.RandomState(1)
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ii = np.array([0, 4, 1, 2, 5], dtype=np.int32)
    dd = rng.randn(5)
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    i32, i64, u32, f64 = C.c_int32, C.c_int64, C.c_uint32, C.c_double
    y = np.array([1.0, -1.0, 1.0])
    V, K = _capi.BANK_CURVE_VALUES, _capi.BANK_CURVE_COUNTS
    out = np.full(64 * 40 * V, 7.25)
    counts = np.full(64 * 40 * K, 7, dtype=np.int64)
    aout = np.full(64 * 40 * 3, 7.25)
    pairs = np.full(64 * 40 * 3, 7, dtype=np.int64)
    masks = lambda *a: np.array(a, dtype=np.uint32)  # noqa: E731

    def call(n_=n, d_=d, ip_=ip, y_=y, w=None, g=None, G=2, s=None, U=0, o=out, cn=counts,
             ao=aout, pr=pairs):
        return lib.spfm_bank_group_curve(eng._h, n_, d_, p(ip_, i64), p(ii, i32), p(dd, f64),
                                         p(y_, f64), 0, p(w, f64), p(g, i32), G, p(s, u32), U,
                                         p(o, f64), p(cn, i64), p(ao, f64), p(pr, i64))

    def untouched():
        return ((out == 7.25).all() and (counts == 7).all() and (aout == 7.25).all()
                and (pairs == 7).all())

    def expect(rc, code, text):
        msg = lib.spfm_last_error(eng._h).decode()
        assert rc == code and text in msg, (rc, msg)
        assert untouched()  # refused before the first write

    INV, UNS = _capi.SPFM_ERR_INVALID, _capi.SPFM_ERR_UNSUPPORTED
    ids = lambda *a: np.array(a, dtype=np.int32)  # noqa: E731
    try:
        expect(call(), INV, "no bank set")
        eng.bank_set(np.array([0, k, 2 * k]), [2], np.zeros((1, d, 2 * k)), np.ones(2 * k),
                     np.zeros((d, F)))
        expect(call(y_=None), INV, "NULL")
        expect(call(g=ids(0, 2, 1)), INV, "group id 2 of row 1")
        expect(call(g=ids(0, -1, 1)), INV, "group id -1")
        expect(call(w=np.array([1.0, -0.5, 1.0])), INV, "negative or not finite")
        expect(call(w=np.array([1.0, np.nan, 1.0])), INV, "negative or not finite")
        expect(call(G=0), INV, "must be >= 1")
        expect(call(d_=d + 1), INV, "the bank has d = %d" % d)
        expect(call(ip_=ip + 1), INV, "bank_group_curve")
        expect(call(G=_capi.BANK_MAX_GROUPS + 1), UNS,
               "SPFM_BANK_MAX_GROUPS = %d" % _capi.BANK_MAX_GROUPS)
        expect(call(s=masks(1, 2, 1, 2), U=0), INV, "U must be >= 1")
        expect(call(s=np.ones(2 * 33, dtype=np.uint32), U=_capi.BANK_MAX_SETS + 1), UNS,
               "SPFM_BANK_MAX_SETS = %d" % _capi.BANK_MAX_SETS)
        expect(call(s=masks(1, 2, 1, 4), U=2), INV, "set 1 of member 1 names a group at or above")
        expect(call(o=None), INV, "NULL")  # out is required, whatever else is given
        # the scratch budget counts this walk's block records: 96 bytes beside the AUC walk's 40
        eng.bank_set(np.arange(65), [2], np.zeros((1, d, 64)), np.ones(64), np.zeros((d, 64)))
        big = 1 << 21
        import re

        def refused_bytes():
            rc = call(n_=big, ip_=np.zeros(big + 1, dtype=np.int64), y_=np.ones(big))
            expect(rc, UNS, "bytes, above SPFM_BANK_AUC_MAX_BYTES = %d" % _capi.BANK_AUC_MAX_BYTES)
            return int(re.search(r"is (\d+) bytes", lib.spfm_last_error(eng._h).decode()).group(1))

        per_member = 12 * big + (40 + 96) * (big // _capi.BANK_RANK_BLOCK) * 2  # U = G = 2
        assert refused_bytes() == 9 * big * 64 + 4 * big + 5 * per_member
        monkeypatch.setenv("SPFM_BANK_AUC_BATCH", "1")
        assert refused_bytes() == 9 * big * 64 + 4 * big + 1 * per_member
        monkeypatch.delenv("SPFM_BANK_AUC_BATCH")
        # valid calls.  n = 0: NaN and zeros, F x U x 11 values and no more
        eng.bank_set(np.array([0, k, 2 * k]), [2], np.zeros((1, d, 2 * k)), np.ones(2 * k),
                     np.zeros((d, F)))
        assert call(n_=0, y_=None, G=3) == 0
        tab = out[:F * 3 * V].reshape(F, 3, V)
        assert np.isnan(tab[:, :, [0, 1, 2, 5, 6]]).all()
        assert (tab[:, :, [3, 4, 7, 8, 9, 10]] == 0).all() and (out[F * 3 * V:] == 7.25).all()
        assert (counts[:F * 3 * K] == 0).all() and (counts[F * 3 * K:] == 7).all()
        atab = aout[:F * 9].reshape(F, 3, 3)
        assert np.isnan(atab[:, :, 0]).all() and (atab[:, :, 1:] == 0).all()
        assert (aout[F * 9:] == 7.25).all()
        assert (pairs[:F * 9] == 0).all() and (pairs[F * 9:] == 7).all()
        # every score is 0 (zero parameters): one run.  counts NULL and no AUC table are accepted
        for a in (out, aout):
            a[:] = 7.25
        for a in (counts, pairs):
            a[:] = 7
        kw = dict(y_=np.array([1.0, -1.0, -1.0]), g=ids(0, 0, 1), s=masks(1, 3, 2, 3), U=2)
        assert call(cn=None, ao=None, pr=None, **kw) == 0
        tab = out[:2 * 2 * V].reshape(2, 2, V).copy()
        assert (out[2 * 2 * V:] == 7.25).all() and (counts == 7).all() and (aout == 7.25).all()
        assert (pairs == 7).all()
        #                 ap      f1   thr  tp fp  ks  thr  tp fp  W+ W-
        assert tab[0, 0].tolist() == [0.5, 2 / 3.0, 0.0, 1, 1, 0.0, 0.0, 1, 1, 1, 1]
        assert tab[0, 1].tolist() == [1 / 3.0, 0.5, 0.0, 1, 2, 0.0, 0.0, 1, 2, 1, 2]
        assert np.isnan(tab[1, 0, [0, 1, 2, 5, 6]]).all()
        assert tab[1, 0, [3, 4, 7, 8, 9, 10]].tolist() == [0, 0, 0, 0, 0, 1]
        assert not np.signbit(tab[0, :, [2, 6]]).any()
        # the same with every table: the curve's values do not move, the AUC's are group_auc's
        assert call(**kw) == 0
        assert np.array_equal(out[:2 * 2 * V].reshape(2, 2, V), tab, equal_nan=True)
        assert counts[:24].reshape(2, 2, K).tolist() == [
            [[1, 1, 1, 1, 1, 1], [1, 2, 1, 2, 1, 2]], [[0, 1, 0, 0, 0, 0], [1, 2, 1, 2, 1, 2]]]
        assert pairs[:12].reshape(2, 2, 3).tolist() == [[[1, 1, 1], [2, 1, 2]],
                                                        [[0, 0, 1], [2, 1, 2]]]
        want_a, want_p = np.full(12, 7.25), np.full(12, 7, dtype=np.int64)
        assert lib.spfm_bank_group_auc(eng._h, n, d, p(ip, i64), p(ii, i32), p(dd, f64),
                                       p(kw["y_"], f64), 0, None, p(kw["g"], i32), 2,
                                       p(kw["s"], u32), 2, p(want_a, f64), p(want_p, i64)) == 0
        assert np.array_equal(aout[:12], want_a, equal_nan=True) and (pairs[:12] == want_p).all()
        assert (aout[12:] == 7.25).all() and (pairs[12:] == 7).all() and (counts[24:] == 7).all()
        # weighted: counts and pairs are not written
        counts[:] = 7
        pairs[:] = 7
        assert call(w=np.array([2.0, 1.0, 0.0]), y_=np.array([1.0, -1.0, -1.0])) == 0
        assert (counts == 7).all() and (pairs == 7).all()
        assert out[:V].tolist() == [2 / 3.0, 0.8, 0.0, 2, 1, 0.0, 0.0, 2, 1, 2, 1]
        assert aout[:3].tolist() == [0.5, 2.0, 1.0]
        info = eng.bank_info()
        assert len(info) == 4 and info["slabs"] == 1
    finally:
        eng.close()


# ---------------------------------------------------------------- 9. the Python callers
def test_cross_validation_selects_by_average_precision():
    import warnings

    from sparsepoly_amd import ModelBank, SparseFactorizationMachineClassifier, cross_validate_path
    from sparsepoly_amd.synth import make_problem

    n = 300
    X, t = make_problem(n, 40, 5, seed=21)
    X = sp.csr_matrix(X)
    X.data = X.data.astype(np.float32).astype(np.float64)
    labels = np.where(np.asarray(t) > np.quantile(t, 0.8), "yes", "no")
    ypm = np.where(labels == "yes", 1.0, -1.0)
    base = SparseFactorizationMachineClassifier(
        solver="pbcd", loss="logistic", regularizer="omegacs", schedule="colored", max_iter=4,
        tol=0, random_state=5, beta=1e-3, gamma=1e-3, alpha=1e-3, n_components=4, precision="f32")
    grid = dict(gamma=[1e-3, 30.0])
    names = ("auc", "average_precision", "ks")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = cross_validate_path(base, X, labels, cv=3, rank_metrics=names,
                                  select="average_precision", **grid)
        only = cross_validate_path(base, X, labels, cv=3, rank_metrics=("auc",), select="auc",
                                   **grid)
        clf = base.fit(X, labels)
    K = 3
    assert set(res.test_) == {"loss", "sign_error"} | set(names)
    assert res.info_ == dict(banks=1, passes=2, members=[6])
    assert res.info_["passes"] == 2 * res.info_["banks"]
    clones = [e for row in res.estimators_ for e in row]
    held = np.tile(np.arange(K), 2)
    own = held[:, None] == np.arange(K)[None, :]
    sets = np.stack([own, ~own], axis=1)
    with ModelBank(clones) as bank:
        curve = bank.group_curve(X, ypm, groups=res.fold_, n_groups=K, sets=sets)
        auc = bank.group_auc(X, ypm, groups=res.fold_, n_groups=K, sets=sets)
    by_hand = dict(auc=auc["auc"], average_precision=curve["average_precision"], ks=curve["ks"])
    for m in names:
        assert not np.isnan(by_hand[m]).any()
        assert (res.test_[m] == by_hand[m][:, 0].reshape(2, K)).all(), m
        assert (res.train_[m] == by_hand[m][:, 1].reshape(2, K)).all(), m
        np.testing.assert_array_equal(res.mean_test_[m], res.test_[m].mean(axis=1))
        np.testing.assert_array_equal(res.std_test_[m], res.test_[m].std(axis=1))
    assert res.best_index_ == int(np.argmax(res.mean_test_["average_precision"]))
    assert res.best_params_ == res.params[res.best_index_]
    # rank_metrics=("auc",): the same fits, the AUC call's own table, every other field as it was
    assert set(only.test_) == {"loss", "sign_error", "auc"}
    assert only.info_ == dict(banks=1, passes=2, members=[6])
    assert only.best_index_ == int(np.argmax(only.mean_test_["auc"]))
    assert (only.fold_ == res.fold_).all() and only.params == res.params
    for m in only.test_:
        np.testing.assert_array_equal(only.test_[m], res.test_[m])
        np.testing.assert_array_equal(only.train_[m], res.train_[m])
        np.testing.assert_array_equal(only.mean_test_[m], res.mean_test_[m])
    # the classifier's own methods: the one-set table of the one-member bank
    w = np.random.RandomState(1).rand(n) + 0.5
    with ModelBank([clf]) as solo:
        tabs = {None: solo.group_curve(X, ypm), "w": solo.group_curve(X, ypm, sample_weight=w)}
    for key, sw in ((None, None), ("w", w)):
        tab = {k_: v[0, 0] for k_, v in tabs[key].items() if k_ != "counts"}
        assert clf.average_precision(X, labels, sample_weight=sw) == tab["average_precision"]
        assert 0.2 < tab["average_precision"] <= 1.0
        for by, value in (("f1", "best_f1"), ("ks", "ks")):
            op = clf.operating_point(X, labels, by=by, sample_weight=sw)
            assert op == dict(threshold=tab[by + "_threshold"], value=tab[value],
                              tp=tab[by + "_tp"], fp=tab[by + "_fp"],
                              pos_weight=tab["pos_weight"], neg_weight=tab["neg_weight"])
            # the threshold does what it says on these rows
            s = clf.decision_function(X)
            ones = np.ones(n) if sw is None else sw
            assert ones[(s >= op["threshold"]) & (ypm > 0)].sum() == pytest.approx(op["tp"])
            assert ones[(s >= op["threshold"]) & (ypm < 0)].sum() == pytest.approx(op["fp"])
