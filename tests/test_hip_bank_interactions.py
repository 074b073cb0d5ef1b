"""Consensus interactions over a model bank: ``ModelBank.
interaction_frequency_stats`` / ``stable_interactions`` / ``top_stable_interactions`` /
``interaction_counts`` and ``interactions.stability_selection`` against the dense NumPy restatement
``restate_bank_counts``.  Members with small-integer parameters make every ``W_f`` and every sum
exact in f64, so those cases compare with ``==``."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from test_ranking_host import all_subsets, fm

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 30, 33)  # padding to 4, more than one chunk of 32 components


def _integer_members(d_u, F, seed=0):
    """F members (``fit_lower='augment'``: one dummy column after the real ones) with entries in
    {-2..2} over d_view = d_u + 5 real features, exactly d_u of them active in some member (5
    inactive in every member) and the dummy column, outside the default view, active in the last;
    member 0 lives on the lower half of the active features and member 1 on the upper half
    (disjoint supports: the skip mask), member 2 is all zero."""
    rng = np.random.RandomState(seed + 100 * d_u + F)
    dv = d_u + 5
    active = np.sort(rng.choice(dv, size=d_u, replace=False))
    halves = [active] if F == 1 else [active[:d_u // 2], active[d_u // 2:]]
    ests = []
    for f in range(F):
        k = KS[(f + d_u) % len(KS)]
        P = np.zeros((k, dv + 1))
        cols = halves[f] if f < len(halves) else active
        if f != 2:
            P[:, cols] = rng.randint(-2, 3, (k, len(cols))) * (rng.rand(k, len(cols)) < 0.4)
        if f < len(halves):
            P[0, cols[(P[:, cols] == 0).all(axis=0)]] = 1.0  # every active feature is stored
        if f == F - 1:
            P[0, dv] = 2.0
        est = fm(2, k, dv, fit_lower="augment", fit_linear=False)
        est.P_, est.lams_ = P[None], rng.choice([-1.0, 1.0], size=k)
        ests.append(est)
    return ests, dv


def _restate(ests, dv, tol):
    from sparsepoly_amd.interactions import restate_bank_counts

    blocks = [(e.P_ if e.P_.ndim == 2 else e.P_[-1])[:, :dv] for e in ests]  # the degree-2 block
    return restate_bank_counts(blocks, [e.lams_ for e in ests], tol)


def _assert_list(got, ref, min_count):
    rows, cols = np.nonzero(ref["count"] >= min_count)  # row-major: sorted by (row, col)
    np.testing.assert_array_equal(got[0], rows)
    np.testing.assert_array_equal(got[1], cols)
    for a, name in zip(got[2:], ("count", "n_pos", "sum")):
        np.testing.assert_array_equal(a, ref[name][rows, cols])


@pytest.mark.parametrize("F", [1, 2, 5, 64])
@pytest.mark.parametrize("d_u", [1, 63, 64, 65, 130])
def test_exact_against_numpy(d_u, F):
    from sparsepoly_amd import ModelBank

    ests, dv = _integer_members(d_u, F)
    with ModelBank(ests) as bank:
        for tol in (0.0, 2.0):  # 2.0 occurs as a value: the strict >
            ref = _restate(ests, dv, tol)
            if tol and d_u > 1:  # (a property of the inputs: the threshold sits on a value)
                assert any((np.triu(np.abs(e.P_[0].T @ (e.lams_[:, None] * e.P_[0]))[:dv, :dv], 1)
                            == tol).any() for e in ests)
            stats = bank.interaction_frequency_stats(tol)
            np.testing.assert_array_equal(stats["histogram"], ref["histogram"])
            np.testing.assert_array_equal(stats["per_member"], ref["per_member"])
            assert stats["n_pairs"] == dv * (dv - 1) // 2 == stats["histogram"].sum()
            for min_count in sorted({1, (F + 1) // 2, F}):
                _assert_list(bank.stable_interactions(min_count, tol), ref, min_count)
        wide = bank.interaction_frequency_stats(2.0, include_augmented=True)
        np.testing.assert_array_equal(wide["histogram"], _restate(ests, dv + 1, 2.0)["histogram"])
        q = np.arange(dv, dtype=np.int32)
        pt = bank.interaction_counts(q, q[::-1], tol=2.0)  # both orders, the diagonal
        full = {n: ref[n] + ref[n].T for n in ("count", "n_pos", "sum")}
        for name in full:
            np.testing.assert_array_equal(pt[name], full[name][q, q[::-1]])


@pytest.fixture(scope="module")
def gaussian():
    """five Gaussian members (k = 5, 30, 33, 4, 1) with sparse columns over d = 150, 130 active"""
    rng = np.random.RandomState(7)
    ests = []
    for f, k in enumerate((5, 30, 33, 4, 1)):
        est = fm(2, k, 150, fit_linear=False, seed=f)
        est.P_[:, :, rng.rand(150) < 0.3] = 0.0
        est.P_[:, :, 130:] = 0.0
        ests.append(est)
    return ests


def test_partition_independence_and_repeats(gaussian):
    from sparsepoly_amd import ModelBank

    with ModelBank(gaussian) as bank:
        base = bank.stable_interactions(1, 0.05)
        stats = bank.interaction_frequency_stats(0.05)
        assert len(base[0]) > 64 * 64
        for budget in (1, 0):
            again = bank.stable_interactions(1, 0.05, tile_budget=budget)
            for a, b in zip(base, again):
                np.testing.assert_array_equal(a, b)
            s2 = bank.interaction_frequency_stats(0.05, tile_budget=budget)
            np.testing.assert_array_equal(stats["histogram"], s2["histogram"])
            np.testing.assert_array_equal(stats["per_member"], s2["per_member"])


def test_a_member_carries_the_bits_of_its_own_calls(gaussian):
    from sparsepoly_amd import ModelBank

    rng = np.random.RandomState(3)
    rows, cols = rng.randint(0, 150, 500), rng.randint(0, 150, 500)
    for est in gaussian[:3]:
        with ModelBank([est]) as solo:
            np.testing.assert_array_equal(solo.interaction_counts(rows, cols)["sum"],
                                          est.interaction_values(rows, cols))
            own = est.interactions(0.1)  # the MFMA chain of the one-model pass
            r, c, count, _, sums = solo.stable_interactions(1, 0.1)
            np.testing.assert_array_equal((r, c), (own.row, own.col))
            np.testing.assert_array_equal(sums, own.data)
            assert (count == 1).all()
    with ModelBank(gaussian) as bank:
        for tol in (0.0, 0.1):
            per = bank.interaction_frequency_stats(tol)["per_member"]
            assert per.tolist() == [e.interaction_stats(tol)["nnz"] for e in gaussian]


def test_gaussian_bank_against_numpy(gaussian):
    """tol = 0: exact counts; a sum is off by at most the roundings one of its terms goes through
    (k_max products and additions of the chain, F additions over the members, the product with
    lams and one to spare) times the sum of the terms' magnitudes."""
    from sparsepoly_amd import ModelBank

    ref = _restate(gaussian, 150, 0.0)
    mag = sum(np.abs(e.P_[0]).T @ np.abs(e.P_[0]) for e in gaussian)
    with ModelBank(gaussian) as bank:
        r, c, count, n_pos, sums = bank.stable_interactions(1)
    rows, cols = np.nonzero(ref["count"] >= 1)
    np.testing.assert_array_equal((r, c), (rows, cols))
    np.testing.assert_array_equal(count, ref["count"][rows, cols])
    np.testing.assert_array_equal(n_pos, ref["n_pos"][rows, cols])
    bound = (33 + len(gaussian) + 2) * 2.0 ** -53 * mag[rows, cols]
    err = np.abs(sums - ref["sum"][rows, cols])
    print("max err / bound: %.3g" % (err / bound).max())
    assert (err <= bound).all()


def test_refusals(gaussian):
    from sparsepoly_amd import ModelBank

    with pytest.raises(ValueError, match="no degree-2 block"):
        with ModelBank([fm(3, 4, 20, fit_lower=None)]) as b3:
            b3.interaction_frequency_stats()
    bank = ModelBank(gaussian[:2])
    for bad in (0, 3):
        with pytest.raises(ValueError, match="min_count"):
            bank.stable_interactions(bad)
        with pytest.raises(ValueError, match="min_count"):
            bank._engine.bank_interaction_list(0, 150, 0.0, bad, 10)
    for call in (bank.interaction_frequency_stats, lambda t: bank.stable_interactions(1, t),
                 lambda t: bank.interaction_counts([0], [1], t),
                 lambda t: bank._engine.bank_interaction_hist(0, 150, t)):
        with pytest.raises(ValueError, match="tol"):
            call(-1.0)
    with pytest.raises(ValueError, match="out of range"):
        bank.interaction_counts([0], [150])
    n = int(bank.interaction_frequency_stats()["histogram"][1:].sum())
    with pytest.raises(ValueError, match="%d pairs .* max_pairs=%d" % (n, n - 1)):
        bank.stable_interactions(1, max_pairs=n - 1)
    out = [np.full(n, -7, dtype=np.int32) for _ in range(4)] + [np.full(n, -7.0)]
    with pytest.raises(ValueError, match="%d pairs .* capacity %d" % (n, n - 1)):
        bank._engine.bank_interaction_list(0, 150, 0.0, 1, n - 1, out=out)
    assert all((a == -7).all() for a in out)  # a short capacity writes nothing
    bank.close()
    for call in (bank.interaction_frequency_stats, lambda: bank.stable_interactions(1),
                 lambda: bank.top_stable_interactions(3), lambda: bank.interaction_counts([0], [1])):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_explicit_lower_block_all_subsets_and_the_augmented_view():
    from sparsepoly_amd import ModelBank

    e3 = [fm(3, k, 40, fit_lower="explicit", seed=k) for k in (3, 6)]  # block 1 holds degree 2
    with ModelBank(e3) as bank:
        ref = _restate(e3, 40, 0.2)
        got = bank.stable_interactions(1, 0.2)
        np.testing.assert_array_equal(got[2], ref["count"][got[0], got[1]])
        assert len(got[0]) == (ref["count"] >= 1).sum()
    subs = [all_subsets(k, 40, seed=k) for k in (2, 5)]
    with ModelBank(subs) as bank:
        hist = bank.interaction_frequency_stats(0.05)["histogram"]
        np.testing.assert_array_equal(hist, _restate(subs, 40, 0.05)["histogram"])
    aug = [fm(3, 4, 20, fit_lower="augment", seed=1)]  # degree 3: no degree-2 block at all
    with pytest.raises(ValueError, match="no degree-2 block"):
        with ModelBank(aug) as bank:
            bank.interaction_frequency_stats()


def test_top_stable_interactions():
    """integer members: exact sums with many ties in count and |sum|, so the order is tested"""
    from sparsepoly_amd import ModelBank

    ests, dv = _integer_members(65, 5)
    ref = _restate(ests, dv, 1.0)
    rows, cols = np.nonzero(ref["count"] >= 1)
    count, sums = ref["count"][rows, cols], ref["sum"][rows, cols]
    order = np.lexsort((cols, rows, -np.abs(sums), -count))
    with ModelBank(ests) as bank:
        for K in (0, 1, 10, 300, len(rows) + 5):
            r, c, cnt, _, s = bank.top_stable_interactions(K, 1.0)
            keep = order[:K]
            np.testing.assert_array_equal((r, c, cnt, s),
                                          (rows[keep], cols[keep], count[keep], sums[keep]))


def test_stability_selection():
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.interactions import stability_selection
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(200, 30, 5, seed=3)
    est = SparseFactorizationMachineRegressor(solver="pcd", schedule="colored", max_iter=4, tol=0,
                                              random_state=0, gamma=1e-2, beta=1e-3, alpha=1e-3,
                                              n_components=4, precision="f64")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bank = stability_selection(est, sp.csr_matrix(X), y, 3, random_state=0)
    with bank:
        assert bank.n_models == 3 and bank.subsample_masks_.sum(axis=1).tolist() == [100] * 3
        merged = sum(abs(e.interactions(0.0).tocsr()).sign() for e in bank.estimators).tocsr()
        merged.sort_indices()
        want = merged.tocoo()  # sorted by (row, col)
        r, c, count, _, _ = bank.stable_interactions(1)
        np.testing.assert_array_equal((r, c, count), (want.row, want.col, want.data))
        hist = bank.interaction_frequency_stats()["histogram"]
        assert hist[1:].tolist() == [(want.data == v).sum() for v in (1, 2, 3)]
