"""``spfm_interaction_degrees`` / ``spfm_interaction_partners`` and what the estimators build on
them, on the device.  Needs a real MI355X: ``pytest -m gpu``.

Exact cases use integer-valued blocks: every product, sum and order is exact in f64 (and the
block itself in f32), so ids, values, counts, degrees and ``sum_abs`` are compared with ``==``
against the NumPy restatement (``restate_partners`` / ``restate_degrees``, pinned by hand in
``tests/test_partners_host.py``).  Float cases use the bounds of ``tests/test_hip_interactions.py``:
one entry of W is a dot product of length k, forward error at most ``(k + 2) 2^-53 sum_s |p_sj
p_sj'|`` on either side, hence ``2 (k + 2) 2^-53 sum_s |p_sj p_sj'|`` between the device and
NumPy; a row sum of d such entries adds ``d`` roundings: ``2 (d + k + 4) 2^-53`` times the summed
products.  None of the bounds comes from a device run."""
import numpy as np
import pytest
import scipy.sparse as sp
from conftest import load_golden
from test_hip_interactions import PSGD_BATCH, _engine, _live_block, _notebook_fm, _quiet
from test_hip_objective import _problem

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BY = ("abs", "positive", "negative")


def _restate():
    from sparsepoly_amd.interactions import restate_degrees, restate_partners

    return restate_partners, restate_degrees


def _int_block(seed, k, d, amp=3, zero_cols=0.2):
    """Integer entries in [-amp, amp], a share of all-zero columns, random +-1 lams"""
    rng = np.random.RandomState(seed)
    P = rng.randint(-amp, amp + 1, size=(k, d)).astype(np.float64)
    if d > 2:
        P[:, rng.rand(d) < zero_cols] = 0.0
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    return P, lams


def _same(got, want, what):
    for g, w, name in zip(got, want, ("ids", "vals", "counts")):
        assert np.array_equal(g, w), (what, name, g, w)


def _check_partners(eng, P, lams, K, features=None, among=None, by="abs", what="", **part):
    restate_partners, _ = _restate()
    got = eng.interaction_partners(0, features, K, among=among, by=by, **part)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    _same(got, restate_partners(P, lams, K, features, among, by), (what, K, among, by, part))
    return got


def _check_degrees(eng, P, lams, tol, what="", **part):
    _, restate_degrees = _restate()
    got = eng.interaction_degrees(0, tol, **part)
    want = restate_degrees(P, lams, tol)
    assert got["degree"].dtype == np.int64 and got["strongest"].dtype == np.int32
    for key in ("degree", "sum_abs", "max_abs", "strongest"):
        assert np.array_equal(got[key], want[key]), (what, tol, key, got[key], want[key])
    return got


# ------------------------------------------------------------------ 1. exact, shapes
@pytest.mark.parametrize("d", [1, 2, 63, 64, 65, 130])
def test_exact_shapes(d):
    for k in (1, 3, 30, 33, 70):
        P, lams = _int_block(1000 * d + k, k, d)
        for layout in ("P", "Pt"):
            Pl = _live_block(P, lams, layout)
            for precision in ("f32", "f64"):
                what = (d, k, layout, precision)
                eng = _engine(P, lams, layout, precision=precision)
                _check_degrees(eng, Pl, lams, 0.0, what)
                _check_degrees(eng, Pl, lams, 2.0, what)
                _check_partners(eng, Pl, lams, 5, what=what)
                _check_partners(eng, Pl, lams, 1, by="negative", what=what)
                eng.close()


def test_massive_ties():
    """Entries in {-1, 0, 1}, k = 3: W takes seven values, so nearly every comparison is a tie
    and the id order decides.  All-zero columns are queries and (non-)partners."""
    rng = np.random.RandomState(5)
    P = rng.randint(-1, 2, size=(3, 130)).astype(np.float64)
    P[:, [0, 17, 63, 64, 129]] = 0.0
    lams = np.array([1.0, -1.0, 1.0])
    eng = _engine(P, lams)
    for tol in (0.0, 1.0):
        got = _check_degrees(eng, P, lams, tol)
    assert (got["strongest"][[0, 17, 63, 64, 129]] == -1).all()
    for by in BY:
        for K in (1, 10, 128):
            ids, _, counts = _check_partners(eng, P, lams, K, by=by)
            assert (counts[[0, 17, 63, 64, 129]] == 0).all()
            assert not np.isin(ids, [0, 17, 63, 64, 129]).any()
    eng.close()


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_selection_stress(order):
    """d = 400, k = 1.  Ascending keys: every candidate beats everything before it, so every one
    survives and every tile forces a compaction; descending: the first K stay."""
    d = 400
    p = np.arange(1, d + 1) if order == "ascending" else np.arange(d, 0, -1)
    P = p[None].astype(np.float64)
    for lam, by in ((1.0, "abs"), (1.0, "positive"), (-1.0, "negative")):
        lams = np.array([lam])
        eng = _engine(P, lams)
        for K in (1, 10, 128):
            _check_partners(eng, P, lams, K, by=by)
            _check_partners(eng, P, lams, K, by=by, cand_strip=128)  # four lists to merge
        # K larger than the number of admissible partners
        ids, _, counts = _check_partners(eng, P, lams, 128, among=(5, 20), by=by)
        assert set(counts.tolist()) == {14, 15} and (ids[:, 15:] == -1).all()
        other = "negative" if by != "negative" else "positive"
        _, _, counts = _check_partners(eng, P, lams, 10, by=other)
        assert not counts.any()
        _check_degrees(eng, P, lams, 0.0)
        eng.close()


def test_among_features_and_by():
    P, lams = _int_block(77, 5, 200, amp=4)
    lams[:] = [1.0, -1.0, -1.0, 1.0, -1.0]
    eng = _engine(P, lams)
    feats = np.array([7, 7, 150, 0, 199, 64, 63, 7])
    for by in BY:
        _check_partners(eng, P, lams, 10, among=(5, 131), by=by)
        _check_partners(eng, P, lams, 10, features=feats, among=(5, 131), by=by)
        _check_partners(eng, P, lams, 10, features=feats, by=by)
        _check_partners(eng, P, lams, 10, by=by)
        _check_partners(eng, P, lams, 3, among=(130, 200), by=by)
    # the view: features >= n are neither queries nor partners
    n = 150
    got = eng.interaction_partners(0, None, 10, n_features=n)
    restate_partners, restate_degrees = _restate()
    _same(got, restate_partners(P[:, :n], lams, 10), "view")
    deg = eng.interaction_degrees(0, 0.0, n_features=n)
    want = restate_degrees(P[:, :n], lams)
    for key in want:
        assert np.array_equal(deg[key], want[key]), key
    ids, vals, counts = eng.interaction_partners(0, [3, 160, 149], 4, n_features=n)
    assert counts[1] == 0 and (ids[1] == -1).all() and ids.max() < n
    eng.close()


# ------------------------------------------------------------------ 2. partitions change no bit
def test_partition_invariance():
    rng = np.random.RandomState(3)
    P = rng.randn(30, 400)
    P[:, rng.rand(400) < 0.1] = 0.0
    lams = np.where(rng.rand(30) < 0.5, -1.0, 1.0)
    eng = _engine(P, lams)
    ref = None
    for row_slab, cand_strip in ((0, 0), (64, 64), (128, 192)):
        for _ in range(2):
            got = eng.interaction_partners(0, None, 10, row_slab=row_slab, cand_strip=cand_strip)
            got += eng.interaction_partners(0, None, 128, among=(5, 331), by="negative",
                                            row_slab=row_slab, cand_strip=cand_strip)
            ref = got if ref is None else ref
            for a, b in zip(got, ref):
                assert np.array_equal(a, b), (row_slab, cand_strip)
        if row_slab:
            assert eng.get_option("interaction_launches") == -(-400 // row_slab)
    ref = None
    for cand_strip in (0, 64, 192):
        for _ in range(2):
            got = eng.interaction_degrees(0, 0.05, cand_strip=cand_strip)
            ref = got if ref is None else ref
            for key in got:
                assert np.array_equal(got[key], ref[key]), (cand_strip, key)
    assert ref["sum_abs"].min() == 0.0 and ref["sum_abs"].max() > 0.0
    assert eng.get_option("interaction_launches") == 1
    eng.close()


# ------------------------------------------------------------------ 3. the other entries agree
def test_cross_entry_identities():
    rng = np.random.RandomState(8)
    d, k = 300, 30
    P = rng.randn(k, d) * (rng.rand(k, d) < 0.5)
    P[:, rng.rand(d) < 0.15] = 0.0
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    eng = _engine(P, lams)
    for tol in (0.0, 0.1):
        st = eng.interaction_stats(0, tol)
        deg = eng.interaction_degrees(0, tol)
        assert deg["degree"].sum() == 2 * st["nnz"]
    assert deg["max_abs"].max() == st["max_abs"]
    st = eng.interaction_stats(0, 0.0)
    rows, cols, vals = eng.interaction_list(0, 0.0, st["nnz"])
    listed = {(int(r), int(c)): v for r, c, v in zip(rows, cols, vals)}
    ids, pv, counts = eng.interaction_partners(0, None, 7)
    seen = 0
    for j in range(d):
        for q in range(counts[j]):
            jj = int(ids[j, q])
            assert listed[(min(j, jj), max(j, jj))] == pv[j, q], (j, jj)  # same bits
            seen += 1
    assert seen > 1000
    deg = eng.interaction_degrees(0, 0.0)
    assert np.array_equal(np.minimum(deg["degree"], 7), counts)
    ids1, v1, _ = eng.interaction_partners(0, None, 1)
    assert np.array_equal(deg["strongest"], ids1[:, 0])
    assert np.array_equal(deg["max_abs"], np.abs(v1[:, 0]))
    eng.close()


# ------------------------------------------------------------------ 4. floats, derived bounds
def test_float_blocks():
    rng = np.random.RandomState(21)
    d, k, K = 300, 30, 10
    P = rng.randn(k, d)
    P[:, [4, 100, 299]] = 0.0
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    W = P.T @ (lams[:, None] * P)
    bound = 2 * (k + 2) * U * (np.abs(P).T @ np.abs(P))  # per entry
    off = ~np.eye(d, dtype=bool)
    eng = _engine(P, lams)
    deg = eng.interaction_degrees(0, 0.0)
    want_sum = (np.abs(W) * off).sum(axis=1)
    sum_bound = 2 * (d + k + 4) * U * ((np.abs(P).T @ np.abs(P)) * off).sum(axis=1)
    err = np.abs(deg["sum_abs"] - want_sum)
    print("sum_abs: worst fraction of the bound %.3g"
          % (err[sum_bound > 0] / sum_bound[sum_bound > 0]).max())
    assert (err <= sum_bound).all()
    assert (np.abs(deg["max_abs"] - (np.abs(W) * off).max(axis=1)) <= bound.max(axis=1)).all()
    assert np.array_equal(deg["degree"], ((W != 0) & off).sum(axis=1))
    for by, among in (("abs", None), ("positive", (10, 250)), ("negative", None)):
        lo, hi = among or (0, d)
        ids, vals, counts = eng.interaction_partners(0, None, K, among=among, by=by)
        sign = {"abs": None, "positive": 1.0, "negative": -1.0}[by]
        key = (lambda w: np.abs(w)) if sign is None else (lambda w: sign * w)
        worst = 0.0
        for j in range(d):  # every row
            n = counts[j]
            jj = ids[j, :n]
            assert (ids[j, n:] == -1).all() and (vals[j, n:] == 0).all()
            assert len(set(jj.tolist())) == n and (jj != j).all()
            assert ((jj >= lo) & (jj < hi)).all()
            kv = key(vals[j, :n])
            assert (kv > 0).all() and (np.diff(kv) <= 0).all()
            e = np.abs(vals[j, :n] - W[j, jj]) / bound[j, jj]
            worst = max(worst, e.max(initial=0.0))
            assert (e <= 1).all()
            kth = kv[-1] if n == K else 0.0
            rest = np.setdiff1d(np.arange(lo, hi), np.append(jj, j))
            assert (key(W[j, rest]) <= kth + 2 * bound[j, rest]).all(), (by, j)
        print("%s: worst value error %.3g of its bound" % (by, worst))
        assert counts[[4, 100, 299]].sum() == 0
    eng.close()


# ------------------------------------------------------------------ 5. estimator level
def _probe(est, **kw):
    deg = est.interaction_degrees(**kw)
    return (deg["degree"], deg["sum_abs"], deg["max_abs"], deg["strongest"]) + \
        est.top_partners(5, **kw) + est.top_partners(3, among=(10, 70), by="negative", **kw)


@pytest.mark.parametrize("solver,reg", [("pcd", "squaredl12"), ("pbcd", "squaredl21")])
def test_mid_fit_equals_post_fit(solver, reg):
    """The last callback runs after the last epoch: the live image (pbcd: the (d,k) one, while
    ``P_`` is stale) and a fresh engine that receives the fitted ``P_`` hold the same bits."""
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y = _problem(1000, 100, 8, 9)
    seen = []
    est = SparseFactorizationMachineRegressor(
        degree=2, n_components=4, solver=solver, regularizer=reg, beta=1.0, gamma=1e-3,
        max_iter=4, tol=-1, n_calls=1, callback=lambda e: seen.append(_probe(e)) and None,
        random_state=0, precision="f64")
    with _quiet():
        est.fit(X, y)
    assert len(seen) >= 4
    after = _probe(est)
    for a, b in zip(seen[-1], after):
        assert np.array_equal(a, b)
    assert any(not np.array_equal(a, b) for a, b in zip(seen[0], after))  # it trained
    restate_partners, restate_degrees = _restate()
    want = restate_degrees(est.P_[0], est.lams_)
    assert np.array_equal(after[0], want["degree"])
    assert np.array_equal(after[6], np.minimum(want["degree"], 5))


def test_include_augmented():
    z = load_golden("g12_interactions.npz")
    est = _notebook_fm(fit_lower="augment", max_iter=10)
    with _quiet():
        est.fit(z["X"], z["y"])
    P = est.P_[0]
    assert P.shape == (30, 101)
    _, restate_degrees = _restate()
    for flag, Pv in ((False, P[:, :100]), (True, P)):
        dv = Pv.shape[1]
        deg = est.interaction_degrees(include_augmented=flag)
        assert all(v.shape == (dv,) for v in deg.values())
        assert np.array_equal(deg["degree"], restate_degrees(Pv, est.lams_)["degree"])
        assert deg["strongest"].max() < dv
        ids, vals, counts = est.top_partners(4, include_augmented=flag)
        assert ids.shape == (dv, 4) and ids.max() < dv
        assert np.array_equal(counts, np.minimum(deg["degree"], 4))
        assert np.array_equal(ids[:, 0], deg["strongest"])
    assert est.top_partners(2, features=[100], include_augmented=True)[0].shape == (1, 2)
    with pytest.raises(ValueError, match="out of range"):
        est.top_partners(2, features=[100])


def test_all_subsets_and_degree3_lower_block():
    from sparsepoly_amd import SparseAllSubsetsRegressor, SparseFactorizationMachineRegressor

    X, y = _problem(1000, 80, 6, 4)
    _, restate_degrees = _restate()
    est = SparseAllSubsetsRegressor(n_components=4, solver="pcd", regularizer="omegati", beta=1.0,
                                    gamma=1e-2, max_iter=5, tol=-1, random_state=0,
                                    precision="f64")
    fm3 = SparseFactorizationMachineRegressor(degree=3, n_components=4, solver="pcd",
                                              regularizer="omegati", beta=10.0, gamma=1e-3,
                                              max_iter=3, tol=-1, random_state=0, precision="f64")
    for model, block in ((est, lambda m: m.P_), (fm3, lambda m: m.P_[1])):
        with _quiet():
            model.fit(X, y)
        want = restate_degrees(block(model), model.lams_)
        deg = model.interaction_degrees()
        assert np.array_equal(deg["degree"], want["degree"]) and want["degree"].any()
        ids, vals, counts = model.top_partners(6)
        assert np.array_equal(counts, np.minimum(want["degree"], 6))
        assert np.array_equal(ids[:, 0], deg["strongest"])
        assert np.array_equal(np.abs(vals[:, 0]), deg["max_abs"])
    none = SparseFactorizationMachineRegressor(degree=3, n_components=4, fit_lower=None)
    none.P_, none.lams_ = fm3.P_[:1], fm3.lams_
    for call in (none.interaction_degrees, lambda: none.top_partners(3)):
        with pytest.raises(ValueError, match="no degree-2 block.*degree=3"):
            call()


@pytest.mark.parametrize("solver,reg", [("pcd", "squaredl12"), ("pbcd", "squaredl21"),
                                        ("psgd", "squaredl12")])
def test_read_only_estimator_callback(solver, reg, capsys):
    """Two fits, one probed with both calls between all epochs: bit-identical ``P_``, ``w_`` and
    ``verbose`` lines (psgd: one-row minibatches, see ``PSGD_BATCH`` in
    tests/test_hip_interactions.py and DESIGN.md section 14)."""
    from sparsepoly_amd import SparseFactorizationMachineRegressor

    X, y = _problem(300, 60, 8, 9) if solver == "psgd" else _problem(1000, 100, 8, 9)
    fits, logs = [], []
    for probing in (True, False):
        def cb(est):
            if probing:
                deg = est.interaction_degrees()
                _, _, counts = est.top_partners(5)
                assert np.array_equal(counts, np.minimum(deg["degree"], 5))

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
    assert np.array_equal(fits[0].w_, fits[1].w_)
    assert logs[0].count("\n") >= 4 and logs[0] == logs[1]


def test_partner_graph():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.interactions import partner_graph

    P, lams = _int_block(31, 6, 90, amp=5)
    est = SparseFactorizationMachineRegressor(degree=2, n_components=6, fit_linear=False)
    est.P_, est.lams_, est.w_ = P[None], lams, np.zeros(90)
    K = 4
    for kw in (dict(), dict(among=(30, 90), by="positive"), dict(features=[5, 80, 5, 33])):
        G = partner_graph(est, K, **kw)
        assert sp.isspmatrix_csr(G) and G.shape == (90, 90)
        feats = np.unique(kw.get("features", np.arange(90)))
        ids, vals, counts = est.top_partners(K, **dict(kw, features=feats))
        per_row = np.diff(G.indptr)
        assert per_row.max() <= K and per_row.sum() == counts.sum()
        assert np.array_equal(per_row[feats], counts)
        for q, j in enumerate(feats):
            sl = slice(G.indptr[j], G.indptr[j + 1])
            assert np.array_equal(G.indices[sl], ids[q, :counts[q]])
            assert np.array_equal(G.data[sl], vals[q, :counts[q]])


# ------------------------------------------------------------------ 6. W is never stored
def _rank1(d):
    """k = 4, p_0j = 1 + (7919 j mod 100003), the other components zero: W[j, j'] = p_0j p_0j',
    distinct integers whose products (< 2^34) and row sums (< 2^51) are exact."""
    f = 1.0 + (7919 * np.arange(d, dtype=np.int64)) % 100003
    P = np.zeros((4, d))
    P[0] = f
    return P, np.array([1.0, -1.0, 1.0, -1.0]), f


def _rank1_partners(f, J, K):
    top = np.argsort(-f, kind="stable")[:K + 1]
    ids = np.array([[t for t in top if t != j][:K] for j in J], dtype=np.int32)
    return ids, f[np.asarray(J)][:, None] * f[ids]


def _under_a_gib(eng, free0):
    assert 0 < eng.get_option("interaction_scratch_kib") < (1 << 20)
    assert free0 - eng.get_option("free_mem_mib") < 1024


def test_never_stored_degrees_at_100k():
    d = 100_000
    P, lams, f = _rank1(d)
    eng = _engine(P, lams)
    free0 = eng.get_option("free_mem_mib")
    deg = eng.interaction_degrees(0, 0.0)
    _under_a_gib(eng, free0)  # a stored W would be 80 GB
    order = np.argsort(-f, kind="stable")
    first, second = order[0], order[1]
    strongest = np.full(d, first, dtype=np.int32)
    strongest[first] = second
    assert (deg["degree"] == d - 1).all()
    assert np.array_equal(deg["sum_abs"], f * (f.sum() - f))
    assert np.array_equal(deg["max_abs"], f * f[strongest])
    assert np.array_equal(deg["strongest"], strongest)
    thr = float(np.median(f)) * 50_000.5
    got = eng.interaction_degrees(0, thr)["degree"]
    fs = np.sort(f)
    want = d - np.searchsorted(fs, thr / f, side="right") - (f * f > thr)
    assert np.array_equal(got, want)
    eng.close()


def test_never_stored_partners_of_4096_at_100k():
    d = 100_000
    P, lams, f = _rank1(d)
    J = (np.arange(4096) * 24 + 7).astype(np.int32)
    J[:9] = np.argsort(-f, kind="stable")[:9]  # the queries that are their own best partner
    eng = _engine(P, lams)
    free0 = eng.get_option("free_mem_mib")
    ids, vals, counts = eng.interaction_partners(0, J, 8)
    _under_a_gib(eng, free0)
    want_ids, want_vals = _rank1_partners(f, J, 8)
    assert (counts == 8).all()
    assert np.array_equal(ids, want_ids) and np.array_equal(vals, want_vals)
    eng.close()


def test_never_stored_partners_of_all_at_20k():
    d = 20_000
    P, lams, f = _rank1(d)
    eng = _engine(P, lams)
    free0 = eng.get_option("free_mem_mib")
    ids, vals, counts = eng.interaction_partners(0, None, 8)
    _under_a_gib(eng, free0)  # a stored W would be 3.2 GB
    want_ids, want_vals = _rank1_partners(f, np.arange(d), 8)
    assert (counts == 8).all()
    assert np.array_equal(ids, want_ids) and np.array_equal(vals, want_vals)
    assert eng.get_option("interaction_launches") == 5  # slabs of 4096 queries
    eng.release_interaction_scratch()
    assert eng.get_option("interaction_scratch_kib") == 0
    eng.close()


# ------------------------------------------------------------------ 7. errors of the C entries
def test_errors():
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    with pytest.raises(ValueError, match="no parameters"):
        eng.interaction_degrees(0, 0.0)
    with pytest.raises(ValueError, match="no parameters"):
        eng.interaction_partners(0, None, 3)
    eng.close()
    P, lams = _int_block(2, 3, 70)
    eng = _engine(P, lams)
    for o in (-1, 1):
        with pytest.raises(ValueError, match="order index"):
            eng.interaction_degrees(o, 0.0)
        with pytest.raises(ValueError, match="order index"):
            eng.interaction_partners(o, None, 3)
    for J in ([70], [-1], [0, 5, 70]):
        with pytest.raises(ValueError, match="out of range"):
            eng.interaction_partners(0, J, 3)
    for tol in (-1e-300, -1.0, float("nan")):
        with pytest.raises(ValueError, match="tol must be >= 0"):
            eng.interaction_degrees(0, tol)
    for K in (0, -5):
        with pytest.raises(ValueError, match="K must be >= 1"):
            eng.interaction_partners(0, None, K)
    with pytest.raises(NotImplementedError, match="SPFM_INTERACTION_MAX_K = 128"):
        eng.interaction_partners(0, None, 129)
    assert eng.interaction_partners(0, None, 128)[0].shape == (70, 128)
    for among in ((5, 5), (10, 5), (70, 80), (5, 0), (5, -3)):
        with pytest.raises(ValueError, match="empty|outside"):
            eng.interaction_partners(0, None, 3, among=among)
    with pytest.raises(ValueError, match="candidate range"):
        eng.interaction_partners(0, None, 3, among=(-2, 5))
    for by in ("largest", 3, -1):
        with pytest.raises(ValueError, match="by must be"):
            eng.interaction_partners(0, None, 3, by=by)
    for strip in (100, 1, -64):
        with pytest.raises(ValueError, match="multiple of 64"):
            eng.interaction_degrees(0, 0.0, cand_strip=strip)
        with pytest.raises(ValueError, match="multiple of 64"):
            eng.interaction_partners(0, None, 3, cand_strip=strip)
    with pytest.raises(ValueError, match="row_slab"):
        eng.interaction_partners(0, None, 3, row_slab=-1)
    # a failed call leaves the handle usable
    _check_partners(eng, P, lams, 3)
    eng.close()
    # fewer than two active features in view: the empty answers
    for active in ([], [3]):
        P = np.zeros((2, 9))
        P[:, active] = 1.0
        eng = _engine(P, np.ones(2))
        deg = eng.interaction_degrees(0, 0.0)
        assert not deg["degree"].any() and not deg["sum_abs"].any() and not deg["max_abs"].any()
        assert (deg["strongest"] == -1).all()
        ids, vals, counts = eng.interaction_partners(0, None, 4)
        assert (ids == -1).all() and not vals.any() and not counts.any()
        ids, vals, counts = eng.interaction_partners(0, [3, 3, 0], 4, among=(2, 6))
        assert ids.shape == (3, 4) and (ids == -1).all() and not counts.any()
        eng.close()
