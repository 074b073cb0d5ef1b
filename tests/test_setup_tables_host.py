"""The tables every persistent pass runs on -- the entry streams (csrc/spfm_schedule.cpp
build_rowblock_stream / build_pb_stream / build_wide_stream) and the first-fit colouring
(schedule_colored) -- against NumPy restatements of the rules written in that file's comments,
compared bitwise through the host-only entries spfm_stream_build and spfm_schedule_build at the
shapes where such builders go wrong: more row blocks than rows, trailing blocks emptied by the
rounded-up rows per block, steps of 1, 33 and exactly 64 columns, slots of exactly long_thresh
and long_thresh + 1 entries in slots 31 / 32 / 63, empty columns and steps, ties of the balanced
slot groups, the previous-step flags at step 0 and across a gap of one step.  No GPU: this pins
the host builders, which tests/test_hip_setup_tables.py then holds the device kernels to."""
import numpy as np
import pytest

from sparsepoly_amd import _capi
from sparsepoly_amd.engine import stream_build
from sparsepoly_amd.schedule import build_schedule


# ------------------------------------------------------------------------------- structures
class Structure(object):
    """A canonical CSC structure (n rows; cols[j] = the ascending rows of column j), a visiting
    order and step boundaries."""

    def __init__(self, n, cols, batch_ptr, order=None):
        self.n, self.d = int(n), len(cols)
        cols = [np.asarray(sorted(c), dtype=np.int32) for c in cols]
        self.indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
        self.indices = (np.concatenate(cols) if self.indptr[-1] else np.zeros(0)).astype(np.int32)
        self.order = np.arange(self.d, dtype=np.int32) if order is None \
            else np.asarray(order, dtype=np.int32)
        self.batch_ptr = np.asarray(batch_ptr, dtype=np.int32)
        assert self.batch_ptr[0] == 0 and self.batch_ptr[-1] == self.d
        assert sorted(self.order) == list(range(self.d))
        for b in range(len(self.batch_ptr) - 1):   # a step's columns share no row
            rows = np.concatenate([self.col(j) for j in self.step(b)] + [np.zeros(0, np.int32)])
            assert len(rows) == len(np.unique(rows)), b

    nnz = property(lambda self: int(self.indptr[-1]))
    nb = property(lambda self: len(self.batch_ptr) - 1)

    def col(self, j):
        return self.indices[self.indptr[j]:self.indptr[j + 1]]

    def step(self, b):
        return self.order[self.batch_ptr[b]:self.batch_ptr[b + 1]]

    def csr(self, seed=0):
        """The matrix with small-integer values (exact in every storage type) and targets."""
        import scipy.sparse as sp

        rng = np.random.RandomState(seed)
        data = rng.randint(1, 4, size=self.nnz).astype(np.float64) * rng.choice([-1.0, 1.0], self.nnz)
        X = sp.csc_matrix((data, self.indices, self.indptr), shape=(self.n, self.d)).tocsr()
        X.sort_indices()
        return X, rng.randint(-3, 4, size=self.n).astype(np.float64)


def modular(n, d, batch_ptr, order=None):
    """Column j holds the rows = j (mod d): all columns are row-disjoint, any steps are valid."""
    return Structure(n, [np.arange(j, n, d) for j in range(d)], batch_ptr, order)


def dealt(n, batch_ptr, sizes, seed):
    """Every step deals the shuffled rows to its columns (sizes[j] rows to column j): disjoint
    inside a step, shared at random between steps -- so the previous-step flags vary."""
    rng = np.random.RandomState(seed)
    cols = []
    for b in range(len(batch_ptr) - 1):
        rows, at = rng.permutation(n), 0
        for j in range(batch_ptr[b], batch_ptr[b + 1]):
            cols.append(rows[at:at + sizes[j]])
            at += sizes[j]
        assert at <= n
    return Structure(n, cols, batch_ptr)


def long_slots(long_thresh=16):
    """One step of 64 columns over two row blocks of 200 rows: slot 31 holds exactly long_thresh
    entries in block 0 and one more in block 1, slots 32 and 63 the other way round; every other
    slot one entry per block."""
    per = {31: (long_thresh, long_thresh + 1), 32: (long_thresh + 1, long_thresh),
           63: (long_thresh + 1, long_thresh)}
    at, cols = [0, 200], []
    for q in range(64):
        rows = []
        for g, m in enumerate(per.get(q, (1, 1))):
            rows += list(range(at[g], at[g] + m))
            at[g] += m
        cols.append(rows)
    assert at[0] <= 200 and at[1] <= 400
    return Structure(400, cols, [0, 64])


def flag_rows():
    """Three steps of two columns.  Row 0 sits in steps 0, 1, 2 (flagged in 1 and 2), rows 5 and 6
    in steps 1, 2 (flagged in 2), rows 1 and 3 in steps 0 and 2 only (a gap of one step: not
    flagged), rows 2, 4, 10 in step 0 only; row 9, 11 nowhere."""
    return Structure(12, [[0, 1, 2], [3, 4, 10], [0, 5], [6], [0, 1, 5, 7], [3, 6, 8]], [0, 2, 4, 6])


def empty_columns():
    """Step 0: an empty column mid-step and one as the last slot; step 1: empty columns only."""
    cols = [[0, 5, 9], [], [1, 2], [], [], [], [], [], [0, 3], [4, 5, 6], [7], [2, 8]]
    return Structure(11, cols, [0, 4, 8, 12])


def dense_column():
    """Column 0 is present in all 50 rows (a step of its own); the others are row-disjoint."""
    return Structure(50, [np.arange(50)] + [np.arange(j, 50, 7) for j in range(5)], [0, 1, 6])


def group_shapes(seed=3):
    """Steps of 3, 2, 64 and 4 columns: the 3-column step lies two steps before the 64-column
    one (its slot map has 64 slots, 61 of them without entries), the last two steps have no
    step b + 2.  Column sizes vary, so the balanced map differs from the fixed one."""
    bp = [0, 3, 5, 69, 73]
    sizes = np.random.RandomState(seed).randint(0, 9, size=73)
    sizes[[0, 1, 2]] = [40, 3, 17]
    return dealt(700, bp, sizes, seed)


def tied_groups():
    """Two steps of 20 columns, every column one entry in every row block (G = 4, 40 rows per
    block... 160 rows): all counts tie, so both tie rules (by slot, by group) decide alone."""
    cols = [[g * 40 + q for g in range(4)] for q in range(20)] * 2
    return Structure(160, cols, [0, 20, 40])


# name -> (structure, workgroups).  Steps of at most 64 columns: all three stream kinds apply.
STREAM_CASES = {
    "more_blocks_than_rows": (modular(40, 30, [0, 13, 30]), 64),
    "trailing_blocks_empty_9_4": (modular(9, 5, [0, 2, 5]), 4),
    "trailing_blocks_empty_65_64": (modular(65, 7, [0, 7]), 64),
    "short_last_block_ragged_grid": (modular(1003, 37, [0, 1, 34, 37]), 7),
    "steps_of_1_33_64": (modular(300, 98, [0, 1, 34, 98], np.random.RandomState(1).permutation(98)), 6),
    "one_step": (modular(90, 20, [0, 20]), 3),
    "two_steps": (dealt(64, [0, 5, 9], [3] * 9, 2), 5),
    "long_slots_31_32_63": (long_slots(16), 2),
    "empty_columns_and_step": (empty_columns(), 3),
    "all_zero": (Structure(14, [[]] * 6, [0, 2, 6]), 4),
    "dense_column": (dense_column(), 8),
    "previous_step_flags": (flag_rows(), 3),
    "group_shapes": (group_shapes(), 9),
    "group_shapes_owner_rounds": (group_shapes(4), 5),
    "tied_groups": (tied_groups(), 4),
}
# wide steps (more than 64 columns): the wide stream only
WIDE_CASES = {
    "wide_65_512": (modular(1300, 577, [0, 65, 577]), 5),
    "wide_flags": (dealt(900, [0, 70, 71, 200], np.r_[[4] * 70, [9], [5] * 129], 5), 64),
}


# ------------------------------------------------------------------ NumPy restatements: streams
def rows_per(n, G):
    return max((n + G - 1) // G, 1)


def _entries(s, skip=None):
    """Per CSC entry in the stream: its position ii, step b, slot q, row -- and touched[row, b]
    over ALL entries (a skipped entry still marks its row as touched by its step)."""
    pos_of = np.empty(s.d, dtype=np.int64)
    pos_of[s.order] = np.arange(s.d)
    col_of = np.repeat(np.arange(s.d), np.diff(s.indptr))
    pos = pos_of[col_of]
    b = np.searchsorted(s.batch_ptr, pos, side="right") - 1
    q = pos - s.batch_ptr[b]
    ii = np.arange(s.nnz)
    touched = np.zeros((s.n, s.nb + 1), dtype=bool)   # column nb = "step -1": never touched
    touched[s.indices, b] = True
    keep = np.ones(s.nnz, dtype=bool) if skip is None else np.asarray(skip) == 0
    return ii[keep], b[keep], q[keep], s.indices[keep].astype(np.int64), touched


def _exclusive(cnt):
    return np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)


def ref_rowblock(s, G, long_thresh, skip=None):
    """spfm_schedule.cpp:619-624.  Entries sorted by (row block, step, slot, row); sp[(g*nb +
    b)*65 + q] = first entry of slot q; lmask bit q of (g, b) set iff the slot holds MORE than
    long_thresh entries."""
    ii, b, q, row, _ = _entries(s, skip)
    g = row // rows_per(s.n, G)
    perm = np.lexsort((row, q, b, g))
    cnt = np.zeros(G * s.nb * 65 + 1, dtype=np.int64)
    np.add.at(cnt, (g * s.nb + b) * 65 + q, 1)
    lmask = np.zeros(G * s.nb * 2, dtype=np.uint32)
    for gb in range(G * s.nb):
        for slot in range(64):
            if cnt[gb * 65 + slot] > long_thresh:
                lmask[gb * 2 + slot // 32] |= np.uint32(1 << (slot % 32))
    return dict(sp=_exclusive(cnt), src=ii[perm].astype(np.int32), lmask=lmask, n_entries=len(ii))


def ref_pbcd(s, G, NG, balance, skip=None):
    """spfm_schedule.cpp:687-704.  Per (row block, step) the slots below min(64, max(ncols(b),
    ncols(b+2))) are dealt to NG groups of at most 64 / NG: fixed map q -> (q % NG, q / NG), or
    balanced -- slots by descending entry count, ties by slot, each to the group with the fewest
    entries that still has room, ties by group.  Entries sorted by (block, step, group, t, row);
    meta = t | 0x80 if step b-1 touched the row; tab unused = 0xFF."""
    QM = 64 // NG
    ii, b, q, row, touched = _entries(s, skip)
    g = row // rows_per(s.n, G)
    ncols = np.diff(s.batch_ptr)
    cnt = np.zeros((G, s.nb, 64), dtype=np.int64)
    np.add.at(cnt, (g, b, q), 1)
    tab = np.full((G, max(s.nb, 1), 64), 0xFF, dtype=np.uint8)
    grp_of = np.zeros((G, s.nb, 64), dtype=np.int64)
    t_of = np.zeros((G, s.nb, 64), dtype=np.int64)
    for gg in range(G):
        for bb in range(s.nb):
            nw = min(64, max(ncols[bb], ncols[bb + 2] if bb + 2 < s.nb else 0))
            c = cnt[gg, bb]
            load, used = [0] * NG, [0] * NG
            slots = sorted(range(nw), key=lambda x: (-c[x], x)) if balance else range(nw)
            for slot in slots:
                if balance:
                    r = min((r for r in range(NG) if used[r] < QM), key=lambda r: (load[r], r))
                    t = used[r]
                else:
                    r, t = slot % NG, slot // NG
                used[r] += 1
                load[r] += c[slot]
                tab[gg, bb, r * QM + t] = slot
                grp_of[gg, bb, slot], t_of[gg, bb, slot] = r, t
    grp, t = grp_of[g, b, q], t_of[g, b, q]
    perm = np.lexsort((row, t, grp, b, g))
    gcnt = np.zeros(G * s.nb * (NG + 1) + 1, dtype=np.int64)
    np.add.at(gcnt, (g * s.nb + b) * (NG + 1) + grp, 1)
    meta = (t | np.where(touched[row, b - 1], 0x80, 0)).astype(np.uint8)   # b = 0 reads column -1
    return dict(sp=_exclusive(gcnt), src=ii[perm].astype(np.int32), flags=meta[perm],
                tab=tab.reshape(-1), n_entries=len(ii))


def ref_wide(s, G):
    """spfm_schedule.cpp:834-838.  wbase[b] = sum over earlier steps of (ncols + 1), tot = d + nb;
    wsp[g*tot + wbase[b] + q] = first entry of slot q; hz = step b-1 touched the row."""
    ii, b, q, row, touched = _entries(s)
    g = row // rows_per(s.n, G)
    wbase = np.concatenate([[0], np.cumsum(np.diff(s.batch_ptr) + 1)])
    tot = s.d + s.nb
    assert wbase[-1] == tot
    perm = np.lexsort((row, q, b, g))
    cnt = np.zeros(G * tot + 1, dtype=np.int64)
    np.add.at(cnt, g * tot + wbase[b] + q, 1)
    hz = touched[row, b - 1].astype(np.uint8)
    return dict(sp=_exclusive(cnt), src=ii[perm].astype(np.int32), flags=hz[perm],
                n_entries=len(ii))


def host_stream(kind, s, G, **kw):
    return stream_build(kind, s.n, s.indptr, s.indices, s.order, s.batch_ptr, G, **kw)


def assert_tables_equal(got, want, what=""):
    for name, ref in want.items():
        if name == "n_entries":
            assert got[name] == ref, (what, name, got[name], ref)
        else:
            assert got[name].dtype == ref.dtype and got[name].shape == ref.shape, (what, name)
            bad = np.flatnonzero(got[name] != ref)
            assert bad.size == 0, (what, name, bad[:8], got[name][bad[:8]], ref[bad[:8]])


# ------------------------------------------------------------------------------ stream tests
@pytest.mark.parametrize("name", sorted(STREAM_CASES))
@pytest.mark.parametrize("long_thresh", [16, 48])
def test_rowblock_stream_is_the_written_rule(name, long_thresh):
    s, G = STREAM_CASES[name]
    got = host_stream("rowblock", s, G, long_thresh=long_thresh)
    assert_tables_equal(got, ref_rowblock(s, G, long_thresh), name)
    assert got["n_entries"] == s.nnz


def test_long_slot_bits_sit_where_the_counts_say():
    """Slots of exactly 16 entries are short, of 17 long: bit 31 of the first word, bits 0 and
    31 of the second, per row block."""
    s, G = STREAM_CASES["long_slots_31_32_63"]
    got = host_stream("rowblock", s, G, long_thresh=16)
    assert got["lmask"].tolist() == [0, 0x80000001, 0x80000000, 0]
    assert not host_stream("rowblock", s, G, long_thresh=17)["lmask"].any()
    assert host_stream("rowblock", s, G, long_thresh=15)["lmask"].tolist() == \
        [0x80000000, 0x80000001] * 2
    # a matrix without a long slot
    s, G = STREAM_CASES["more_blocks_than_rows"]
    assert not host_stream("rowblock", s, G, long_thresh=16)["lmask"].any()


@pytest.mark.parametrize("name", sorted(STREAM_CASES))
def test_rowblock_stream_with_a_skip_mask(name):
    s, G = STREAM_CASES[name]
    skip = (np.random.RandomState(7).rand(s.nnz) < 0.3).astype(np.uint8)
    got = host_stream("rowblock", s, G, long_thresh=16, skip=skip)
    assert_tables_equal(got, ref_rowblock(s, G, 16, skip), name)
    assert got["n_entries"] == s.nnz - int(skip.sum())


@pytest.mark.parametrize("name", sorted(STREAM_CASES))
@pytest.mark.parametrize("NG", [8, 16])
@pytest.mark.parametrize("balance", [0, 1])
def test_pbcd_stream_is_the_written_rule(name, NG, balance):
    s, G = STREAM_CASES[name]
    got = host_stream("pbcd", s, G, NG=NG, balance=balance)
    assert_tables_equal(got, ref_pbcd(s, G, NG, balance), name)


@pytest.mark.parametrize("name", ["previous_step_flags", "group_shapes", "two_steps"])
def test_pbcd_stream_skipped_entries_still_touch_their_rows(name):
    s, G = STREAM_CASES[name]
    step = _entries(s)[1]    # the even steps' entries are left out, and a few of the others
    skip = ((step % 2 == 0) | (np.random.RandomState(8).rand(s.nnz) < 0.2)).astype(np.uint8)
    got = host_stream("pbcd", s, G, NG=16, balance=0, skip=skip)
    want = ref_pbcd(s, G, 16, 0, skip)
    assert_tables_equal(got, want, name)
    # the case bites: some entry's row was touched by the previous step through skipped
    # entries only
    ii, b, q, row, touched = _entries(s, skip)
    kept_only = np.zeros((s.n, s.nb + 1), dtype=bool)
    kept_only[row, b] = True
    assert (kept_only[row, b - 1] != touched[row, b - 1]).any()


def test_previous_step_flags_row_by_row():
    s, G = STREAM_CASES["previous_step_flags"]
    for kind, kw, bit in (("pbcd", dict(NG=16, balance=1), 0x80), ("wide", {}, 1)):
        got = host_stream(kind, s, G, **kw)
        row = s.indices[got["src"]]
        col = np.searchsorted(s.indptr, got["src"], side="right") - 1
        step = col // 2
        flagged = sorted((int(r), int(b)) for r, b, f in zip(row, step, got["flags"]) if f & bit)
        assert flagged == [(0, 1), (0, 2), (5, 2), (6, 2)], (kind, flagged)


def test_balanced_groups_break_ties_by_slot_then_by_group():
    s, G = STREAM_CASES["tied_groups"]
    got = host_stream("pbcd", s, G, NG=16, balance=1)
    tab = got["tab"].reshape(G, s.nb, 16, 4)
    # equal counts: slots in order, each to the emptiest group, lowest group first: q -> q % 16
    want = np.full((16, 4), 0xFF)
    for q in range(20):
        want[q % 16, q // 16] = q
    assert (tab == want).all()


@pytest.mark.parametrize("name", sorted(STREAM_CASES) + sorted(WIDE_CASES))
def test_wide_stream_is_the_written_rule(name):
    s, G = STREAM_CASES[name] if name in STREAM_CASES else WIDE_CASES[name]
    assert_tables_equal(host_stream("wide", s, G), ref_wide(s, G), name)


def test_stream_build_rejects_what_the_builders_cannot_index():
    s, G = STREAM_CASES["two_steps"]
    ok = dict(kind="rowblock", n_rows=s.n, indptr=s.indptr, indices=s.indices, order=s.order,
              batch_ptr=s.batch_ptr, groups=G)
    stream_build(**ok)
    for change in (dict(n_rows=s.n - 1) if s.indices.max() == s.n - 1 else dict(n_rows=0),
                   dict(groups=0), dict(order=np.zeros(s.d, dtype=np.int32)),
                   dict(batch_ptr=[0, 5, 8]), dict(indices=s.indices[::-1].copy()),
                   dict(kind="pbcd", NG=12), dict(kind="wide", skip=np.zeros(s.nnz, np.uint8))):
        with pytest.raises(ValueError):
            stream_build(**dict(ok, **change))
    wide, Gw = WIDE_CASES["wide_65_512"]     # steps of more than 64 columns: the wide kind only
    for kind in ("rowblock", "pbcd"):
        with pytest.raises(ValueError):
            host_stream(kind, wide, Gw)


# ------------------------------------------------------------------------- sequential first fit
def ref_first_fit(n, indptr, indices, order, max_batch):
    """Each column in visiting order takes the lowest colour that is absent from its rows and
    whose class holds fewer than max_batch columns; classes in colour order, their columns in
    visiting order."""
    d = len(order)
    present = np.zeros((max(n, 1), d + 1), dtype=bool)   # colours on every row
    full = np.zeros(d + 1, dtype=bool)
    classes = []
    for j in order:
        rows = indices[indptr[j]:indptr[j + 1]]
        blocked = full | present[rows].any(axis=0)
        c = int(np.argmin(blocked))                       # the lowest free colour
        assert not blocked[c] and c <= len(classes)
        if c == len(classes):
            classes.append([])
        classes[c].append(int(j))
        full[c] = len(classes[c]) >= max_batch
        present[rows, c] = True
    out = np.array([j for cl in classes for j in cl], dtype=np.int32)
    bp = np.concatenate([[0], np.cumsum([len(cl) for cl in classes])]).astype(np.int32)
    return out, bp


def host_first_fit(n, indptr, indices, order, max_batch):
    """spfm_schedule_build, SPFM_SCHED_COLORED: (order, batch_ptr)."""
    import types

    X = types.SimpleNamespace(shape=(n, len(order)), indptr=indptr, indices=indices)
    return build_schedule(X, "colored", order, max_batch)


def colouring_matrix(kind, d, seed=0):
    """(n, indptr, indices) of the colouring cases."""
    rng = np.random.RandomState(seed)
    if kind == "diagonal":                  # no conflicts
        n, cols = d, [[j] for j in range(d)]
    elif kind == "shared_row":              # a complete conflict graph
        n, cols = 2, [[0] for _ in range(d)]
    elif kind == "random":                  # a few rows per column, empty columns among them
        n = 2 * d + 3
        cols = [rng.choice(n, size=rng.randint(0, 5), replace=False) for _ in range(d)]
    elif kind == "tall_column":             # a column of more than 256 entries, crowded rows
        n = 700
        cols = [rng.choice(n, size=rng.randint(1, 4), replace=False) for _ in range(d)]
        cols[d // 2] = np.arange(0, 600, 2)                      # 300 entries
        cols = [np.union1d(c, [699]) if j % 3 == 0 else c for j, c in enumerate(cols)]
    else:
        raise ValueError(kind)
    s = Structure(n, cols, [0] + list(range(1, d + 1)))  # (one column per step: always valid)
    return s.n, s.indptr, s.indices


COLOUR_CASES = (
    [("random", d, mb, sh) for d in (1, 255, 256, 257, 600) for mb in (1, 2, 64, 512)
     for sh in (False, True) if not (d == 1 and sh)]
    + [("diagonal", 600, mb, False) for mb in (1, 2, 64, 512)]
    + [("shared_row", 300, 64, False), ("shared_row", 300, 64, True),
       ("tall_column", 300, 64, False), ("tall_column", 300, 2, True)]
)


def visiting_order(d, shuffled):
    order = np.arange(d, dtype=np.int32)
    if shuffled:
        np.random.RandomState(4).shuffle(order)
    return order


@pytest.mark.parametrize("kind,d,max_batch,shuffled", COLOUR_CASES)
def test_host_first_fit_is_the_written_rule(kind, d, max_batch, shuffled):
    n, indptr, indices = colouring_matrix(kind, d)
    order = visiting_order(d, shuffled)
    want = ref_first_fit(n, indptr, indices, order, max_batch)
    got = host_first_fit(n, indptr, indices, order, max_batch)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if kind == "diagonal":      # classes fill to exactly max_batch, in order
        assert np.array_equal(got[0], order)
        assert np.diff(got[1]).tolist() == [max_batch] * (d // max_batch) + \
            ([d % max_batch] if d % max_batch else [])
    if kind == "shared_row":    # more than 64 colours: the second word of the colour bitmaps
        assert len(got[1]) - 1 == d


@pytest.mark.parametrize("d", [4096, 4097])
def test_host_first_fit_around_4096_colours(d):
    n, indptr, indices = colouring_matrix("shared_row", d)
    order = visiting_order(d, False)
    want = ref_first_fit(n, indptr, indices, order, 64)
    got = host_first_fit(n, indptr, indices, order, 64)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(got[1]) - 1 == d


def test_the_new_entries_are_declared_and_loaded():
    header = open(__file__.replace("tests/test_setup_tables_host.py", "include/spfm.h")).read()
    for name in ("spfm_stream_build", "spfm_debug_stream_info", "spfm_debug_stream_tables"):
        assert "int %s(" % name in header and name in _capi.SYMBOLS
    assert '"debug_setup_any_size"' in header
