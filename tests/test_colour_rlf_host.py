"""The RLF colouring ('colored_rlf', SPFM_SCHED_COLORED_RLF), host form, through
spfm_schedule_build (csrc/spfm_schedule.cpp, schedule_rlf).  The rule, restated below in NumPy:
one class at a time; the first member maximises the sum over its rows of the uncoloured columns
on the row, every later member the sum over its rows of the candidates that left the class on
that row; a candidate leaves when it shares a row with a member; ties go to the column that comes
first in indices_feature; a class closes at max_batch members or without candidates.  No GPU."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from sparsepoly_amd import _capi
from sparsepoly_amd.schedule import Schedule, build_schedule


def _csc(X):
    X = sp.csc_matrix(X)
    X.sum_duplicates()
    X.sort_indices()
    return X


def _rows_matrix(n, d, per_row, seed, zipf=False):
    """n rows with per_row entries each"""
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), per_row)
    if zipf:
        p = 1.0 / np.arange(1, d + 1) ** 0.9
        cols = rng.choice(d, size=n * per_row, p=p / p.sum())
    else:
        cols = rng.randint(0, d, size=n * per_row)
    return _csc(sp.csr_matrix((np.ones(n * per_row), (rows, cols)), shape=(n, d)))


def _columns_matrix(n, d, per_col, seed):
    """d columns with per_col distinct rows each"""
    rng = np.random.RandomState(seed)
    indices = np.concatenate([np.sort(rng.choice(n, per_col, replace=False)) for _ in range(d)])
    indptr = np.arange(d + 1, dtype=np.int64) * per_col
    return sp.csc_matrix((np.ones(d * per_col), indices.astype(np.int32), indptr), shape=(n, d))


def rlf_numpy(X, order, max_batch):
    """The rule, word for word.  -> (order, batch_ptr)"""
    n, d = X.shape
    rows = [X.indices[X.indptr[j]:X.indptr[j + 1]] for j in range(d)]
    urow = np.bincount(X.indices, minlength=n).astype(np.int64)
    coloured = np.zeros(d, dtype=bool)           # by visiting position
    out, bp = [], [0]
    while not coloured.all():
        cand = [p for p in range(d) if not coloured[p]]
        wrow = np.zeros(n, dtype=np.int64)
        members = []
        while cand and len(members) < max_batch:
            cnt = wrow if members else urow
            keys = [int(cnt[rows[order[p]]].sum()) for p in cand]
            best = cand[int(np.argmax(keys))]    # argmax: the first maximum = earliest position
            v = rows[order[best]]
            urow[v] -= 1
            coloured[best] = True
            members.append(best)
            hit = np.zeros(n, dtype=bool)
            hit[v] = True
            keep = []
            for p in cand:
                if p == best:
                    continue
                r = rows[order[p]]
                if hit[r].any():
                    wrow[r] += 1
                else:
                    keep.append(p)
            cand = keep
        out += [order[p] for p in sorted(members)]   # visiting order inside a class
        bp.append(len(out))
    return np.array(out, dtype=np.int32), np.array(bp, dtype=np.int32)


def _check_valid(X, order, bp, max_batch):
    d = X.shape[1]
    assert sorted(order.tolist()) == list(range(d))          # a permutation
    assert bp[0] == 0 and bp[-1] == d and np.all(np.diff(bp) >= 1)
    assert np.diff(bp).max() <= max_batch
    for b in range(len(bp) - 1):
        cols = order[bp[b]:bp[b + 1]]
        r = np.concatenate([X.indices[X.indptr[j]:X.indptr[j + 1]] for j in cols])
        assert len(r) == len(np.unique(r)), "batch %d shares a row" % b


def _with_empty_columns(X):
    d = X.shape[1]
    keep = np.ones(d)
    keep[[0, 7, d // 2, d - 1]] = 0
    X = sp.csc_matrix(X @ sp.diags(keep))
    X.eliminate_zeros()
    return _csc(X)


def _cases():
    base = _rows_matrix(200, 60, 3, 0)
    shuffled = np.arange(60, dtype=np.int32)
    np.random.RandomState(3).shuffle(shuffled)
    return {
        "uniform": (base, np.arange(60, dtype=np.int32)),
        "shuffled": (base, shuffled),
        "zipf": (_rows_matrix(300, 60, 3, 1, zipf=True), np.arange(60, dtype=np.int32)),
        "empty_columns": (_with_empty_columns(base), np.arange(60, dtype=np.int32)),
    }


CASES = _cases()


def test_mode_is_in_the_tables():
    assert _capi.SCHEDULES["colored_rlf"] == 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "spfm.h")).read()
    assert "#define SPFM_SCHED_COLORED_RLF 2" in text


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("max_batch", [64, 5])
def test_equals_the_numpy_restatement(name, max_batch):
    X, jf = CASES[name]
    order, bp = build_schedule(X, "colored_rlf", jf, max_batch)
    _check_valid(X, order, bp, max_batch)
    ref_order, ref_bp = rlf_numpy(X, jf, max_batch)
    assert np.array_equal(bp, ref_bp)
    assert np.array_equal(order, ref_order)
    again = build_schedule(X, "colored_rlf", jf, max_batch)          # deterministic
    assert np.array_equal(again[0], order) and np.array_equal(again[1], bp)


def test_shuffled_order_decides_ties():
    # columns with private rows of one length: every key ties, so the classes are the visiting
    # order cut into pieces
    d = 10
    X = sp.csc_matrix((np.ones(2 * d), np.arange(2 * d, dtype=np.int32),
                       2 * np.arange(d + 1, dtype=np.int64)), shape=(2 * d, d))
    jf = np.array([3, 9, 0, 5, 1, 8, 2, 7, 4, 6], dtype=np.int32)
    order, bp = build_schedule(X, "colored_rlf", jf, 4)
    assert np.array_equal(order, jf) and bp.tolist() == [0, 4, 8, 10]


def test_one_dense_row_gives_one_column_per_class():
    d = 17
    rng = np.random.RandomState(2)
    M = (rng.rand(40, d) < 0.1).astype(float)
    M[5, :] = 1.0
    X = _csc(M)
    order, bp = build_schedule(X, "colored_rlf", None, 64)
    _check_valid(X, order, bp, 64)
    assert bp.tolist() == list(range(d + 1))


def test_private_rows_fill_classes_to_the_cap():
    d = 200
    X = sp.csc_matrix((np.ones(3 * d), np.arange(3 * d, dtype=np.int32),
                       3 * np.arange(d + 1, dtype=np.int64)), shape=(3 * d, d))
    order, bp = build_schedule(X, "colored_rlf", None, 64)
    assert np.diff(bp).tolist() == [64, 64, 64, 8]
    assert np.array_equal(order, np.arange(d))


def test_max_batch_one():
    X, jf = CASES["uniform"]
    order, bp = build_schedule(X, "colored_rlf", jf, 1)
    _check_valid(X, order, bp, 1)
    assert len(bp) - 1 == X.shape[1]
    ref = rlf_numpy(X, jf, 1)
    assert np.array_equal(order, ref[0])


def test_fewer_columns_than_the_cap():
    X = _rows_matrix(50, 9, 2, 4)
    order, bp = build_schedule(X, "colored_rlf", None, 64)
    _check_valid(X, order, bp, 64)
    ref = rlf_numpy(X, np.arange(9, dtype=np.int32), 64)
    assert np.array_equal(order, ref[0]) and np.array_equal(bp, ref[1])


def test_schedule_object_round_trip(tmp_path):
    X, jf = CASES["zipf"]
    s = Schedule.build(X, "colored_rlf")
    assert s.mode == "colored_rlf" and s.n_batches >= 1
    path = str(tmp_path / "s.npz")
    s.save(path)
    t = Schedule.load(path)
    assert t.mode == "colored_rlf"
    assert np.array_equal(t.order, s.order) and np.array_equal(t.batch_ptr, s.batch_ptr)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fewer_classes_than_first_fit(seed):
    # 3 000 columns of 100 entries on 40 000 rows: conflict density 0.22 (BASELINE config 2's).
    # The prototype of the rule gave 121 classes against first fit's 142.
    X = _columns_matrix(40000, 3000, 100, seed)
    ff = build_schedule(X, "colored", None, 64)
    rlf = build_schedule(X, "colored_rlf", None, 64)
    _check_valid(X, rlf[0], rlf[1], 64)
    n_ff, n_rlf = len(ff[1]) - 1, len(rlf[1]) - 1
    print("seed %d: first fit %d classes, rlf %d classes" % (seed, n_ff, n_rlf))
    assert n_rlf < n_ff
