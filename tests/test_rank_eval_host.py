"""``sparsepoly_amd.ranking.metrics_from_ranks`` and ``check_rank_lists`` without a device: the
metrics against their definitions written out row by row on hand-made ranks, and the input checks
that are raised before any device use."""
import math

import numpy as np
import pytest
import scipy.sparse as sp


def brute(tptr, ranks, n_eff, k):
    """per row (recall@k, hit@k, ndcg@k, mrr, auc) by the definitions; None for a row without
    targets, auc None where n_eff == |T_b|"""
    out = []
    for b in range(len(tptr) - 1):
        r = [int(x) for x in ranks[tptr[b]:tptr[b + 1]]]
        n = len(r)
        if n == 0:
            out.append(None)
            continue
        hits = [x for x in r if 0 <= x < k]
        recall = len(hits) / n
        dcg = sum(1 / math.log2(x + 2) for x in hits)
        idcg = sum(1 / math.log2(i + 2) for i in range(min(n, k)))
        good = [x for x in r if x >= 0]
        mrr = 1 / (min(good) + 1) if good else 0.0
        others = n_eff[b] - n
        if others == 0:
            auc = None
        else:
            # a target of rank -1 is beaten by every other candidate; position i among the sorted
            # finite targets has i targets ahead of it
            lost = sum(x - i for i, x in enumerate(sorted(good))) + (n - len(good)) * others
            auc = 1 - lost / (n * others)
        out.append((recall, float(bool(hits)), dcg / idcg, mrr, auc))
    return out


# rows: no target | one at rank 0 | ranks k-1 and k | more than k targets | a rank of -1 |
# n_eff == |T_b| | every target a miss
K = 3
RANKS = [[], [0], [K - 1, K], [0, 1, 2, 4, 7], [5, -1, 1], [1, 0], [-1]]
N_EFF = [50, 50, 50, 20, 9, 2, 30]


def _flat():
    tptr = np.concatenate([[0], np.cumsum([len(r) for r in RANKS])])
    ranks = np.array([x for r in RANKS for x in r], dtype=np.int32)
    return tptr, ranks, np.array(N_EFF, dtype=np.int32)


def test_metrics_equal_their_definitions():
    from sparsepoly_amd.ranking import metrics_from_ranks

    tptr, ranks, n_eff = _flat()
    for ks in ((K,), (1, K, 10)):
        got = metrics_from_ranks(tptr, ranks, n_eff, ks)
        assert got["n_rows_scored"] == 6
        per = got["per_row"]
        assert (per["n_targets"] == [len(r) for r in RANKS]).all()
        for k in ks:
            want = brute(tptr, ranks, n_eff, k)
            names = ("recall@%d" % k, "hit@%d" % k, "ndcg@%d" % k, "mrr", "auc")
            for b, w in enumerate(want):
                for i, name in enumerate(names):
                    g = per[name][b]
                    if w is None or w[i] is None:
                        assert np.isnan(g), (b, name)
                    else:
                        assert g == pytest.approx(w[i], abs=1e-15), (b, name)
            for i, name in enumerate(names):
                vals = [w[i] for w in want if w is not None and w[i] is not None]
                assert got[name] == pytest.approx(sum(vals) / len(vals), abs=1e-15), name


def test_metrics_spot_values():
    """the cases whose value can be read off"""
    from sparsepoly_amd.ranking import metrics_from_ranks

    tptr, ranks, n_eff = _flat()
    per = metrics_from_ranks(tptr, ranks, n_eff, (K,))["per_row"]
    name = "recall@%d" % K
    assert np.isnan(per[name][0]) and np.isnan(per["auc"][0]) and np.isnan(per["mrr"][0])
    assert per[name][1] == 1.0 and per["ndcg@%d" % K][1] == 1.0 and per["mrr"][1] == 1.0
    assert per["auc"][1] == 1.0
    assert per[name][2] == 0.5  # rank k - 1 is a hit, rank k is not
    assert per[name][3] == 3 / 5 and per["ndcg@%d" % K][3] == 1.0  # |T_b| > k: the ideal has k
    assert per[name][4] == 1 / 3 and per["mrr"][4] == 0.5  # the -1 is a miss
    assert np.isnan(per["auc"][5]) and per[name][5] == 1.0  # n_eff == |T_b|
    assert per[name][6] == 0.0 and per["mrr"][6] == 0.0 and per["auc"][6] == 0.0


def test_metrics_without_any_target():
    from sparsepoly_amd.ranking import metrics_from_ranks

    got = metrics_from_ranks(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32),
                             np.full(3, 7), (2,))
    assert got["n_rows_scored"] == 0 and np.isnan(got["recall@2"]) and np.isnan(got["auc"])
    with pytest.raises(ValueError, match="ks"):
        metrics_from_ranks(np.zeros(2, dtype=np.int64), np.zeros(0), np.full(1, 7), (0,))
    with pytest.raises(ValueError, match="fit together"):
        metrics_from_ranks(np.array([0, 2]), np.zeros(1), np.full(1, 7))


def _lists(B, C, rows):
    r = np.array([b for b, cs in enumerate(rows) for _ in cs], dtype=np.int64)
    c = np.array([x for cs in rows for x in cs], dtype=np.int64)
    return sp.coo_matrix((np.ones(len(r)), (r, c)), shape=(B, C)).tocsr()


def test_checker_refuses():
    from sparsepoly_amd.ranking import check_rank_lists

    B, C = 3, 100
    T = _lists(B, C, [[5, 7], [], [99]])
    E = _lists(B, C, [[6], [1, 2], [0]])
    check_rank_lists(B, C, T, E)
    # an id >= C, in a matrix that claims the right shape
    bad = sp.csr_matrix((B, C))
    bad.indptr = np.array([0, 1, 1, 1], dtype=np.int32)
    bad.indices = np.array([C], dtype=np.int32)
    bad.data = np.ones(1)
    with pytest.raises(ValueError, match="out of range"):
        check_rank_lists(B, C, bad)
    with pytest.raises(ValueError, match="out of range"):
        check_rank_lists(B, C, T, bad)
    # a wrong shape, either way round
    for wrong in (_lists(B + 1, C, [[1]] * (B + 1)), _lists(B, C + 1, [[C]] * B)):
        with pytest.raises(ValueError, match="shape"):
            check_rank_lists(B, C, wrong)
        with pytest.raises(ValueError, match="shape"):
            check_rank_lists(B, C, T, wrong)
    # a target that is also excluded
    with pytest.raises(ValueError, match="candidate 7 is a target of row 0 and excluded"):
        check_rank_lists(B, C, T, _lists(B, C, [[6, 7], [], []]))
    # 65 targets in a row; 64 pass
    check_rank_lists(B, C, _lists(B, C, [[], range(64), []]))
    with pytest.raises(ValueError, match="row 1 has 65 targets.*cap of 64"):
        check_rank_lists(B, C, _lists(B, C, [[], range(65), []]))


def test_checker_canonicalises_and_leaves_the_input_alone():
    from sparsepoly_amd.ranking import check_rank_lists

    B, C = 2, 10
    # unsorted, with a duplicate, values that would cancel if they were summed as numbers
    T = sp.csr_matrix((np.array([1.0, -1.0, 2.0, 3.0]), np.array([7, 7, 2, 4], dtype=np.int32),
                       np.array([0, 3, 4], dtype=np.int32)), shape=(B, C))
    before = (T.data.copy(), T.indices.copy(), T.indptr.copy())
    Tc, E = check_rank_lists(B, C, T)
    assert E is None
    assert (Tc.indptr == [0, 2, 3]).all() and (Tc.indices == [2, 7, 4]).all()
    assert Tc.has_sorted_indices and (Tc.data == 1).all()
    for a, b in zip(before, (T.data, T.indices, T.indptr)):
        assert (a == b).all()
    # dense and boolean input: the non-zeros are the pattern
    D = np.zeros((B, C), dtype=bool)
    D[1, [9, 0]] = True
    Tc, Ec = check_rank_lists(B, C, D, D[::-1])
    assert (Tc.indptr == [0, 0, 2]).all() and (Tc.indices == [0, 9]).all()
    assert (Ec.indptr == [0, 2, 2]).all()
