"""The device set-up kernels table by table: the entry streams of csrc/spfm_ingest.hip
(device_rowblock_stream, with and without a skip mask, device_pb_stream, device_wide_stream) and
the first-fit colouring of csrc/spfm_colour.hip, at the small edge shapes of
tests/test_setup_tables_host.py.  The option ``debug_setup_any_size`` lets a small problem reach
the device forms; every case asserts the ``*_device_used`` read-out (a device builder that fails
falls back to the host silently), fetches the tables the handle holds
(spfm_debug_stream_tables) and compares every array bitwise with the host builders
(spfm_stream_build), which the host file pins to the written rules.  The same handle then
rebuilds the stream on the host (``stream_device`` = 0) and must read back the same tables: that
checks the read-out itself.  Needs a real MI355X."""
import numpy as np
import pytest
import scipy.sparse as sp

from test_setup_tables_host import (COLOUR_CASES, STREAM_CASES, WIDE_CASES, Structure,
                                    assert_tables_equal, colouring_matrix, host_first_fit,
                                    host_stream, modular, ref_first_fit, ref_rowblock,
                                    visiting_order)

pytestmark = pytest.mark.gpu

# wide steps (more than 64 columns, most of them empty) over the small row counts
WIDE_EDGES = dict(WIDE_CASES)
WIDE_EDGES.update({
    "wide_more_blocks_than_rows": (Structure(
        40, [np.arange(j, 40, 30) if j < 30 else [] for j in range(100)], [0, 70, 100],
        np.random.RandomState(2).permutation(100)), 64),
    "wide_trailing_blocks_empty": (Structure(
        9, [np.arange(j, 9, 5) if j < 5 else [] for j in range(70)], [0, 66, 70]), 4),
    "wide_one_step": (modular(1003, 65, [0, 65]), 7),
    "wide_all_zero": (Structure(14, [[]] * 66, [0, 66]), 4),
})


def _handle(X, y, solver, k, options, precision="f32"):
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, precision)
    eng.set_option("debug_setup_any_size", 1)
    for key, value in options:
        eng.set_option(key, value)
    eng.set_data(X, y)
    d = X.shape[1]
    eng.set_params(0.01 * np.random.RandomState(0).randn(1, k, d), np.zeros(d), np.ones(k))
    eng.configure(solver, "squared", "squaredl12" if solver == "pcd" else "omegacs", 2)
    eng.init_pred(2, True, False)
    return eng


def _install(eng, s):
    from sparsepoly_amd.schedule import Schedule

    eng.install_schedule(Schedule(s.order, s.batch_ptr))


def _epoch(eng, solver, k):
    v = eng.cd_linear_epoch(1.0)
    if solver == "pcd":
        return v + eng.pcd_epoch(0, 2, 5.0, 1e-3, 1.0, np.arange(k, dtype=np.int32))
    return v + eng.pbcd_epoch(0, 2, 1.0, 1e-3, 1.0)


# kind -> (solver, the option that sets its workgroups, its read-out, what says the pass ran)
KINDS = {
    "rowblock": ("pcd", "prb_groups", "stream_device_used", "persistent_active"),
    "pbcd": ("pbcd", "pbprb_groups", "pb_stream_device_used", "pbprb_active"),
    "wide": ("pcd", "pcdw_groups", "wide_stream_device_used", "wide_active"),
}


def _check_stream(kind, s, G, k=3, options=()):
    """Device-built, then host-built on the same handle: both read-outs equal the host entry
    called with the parameters the handle reports."""
    solver, groups_key, used_key, active_key = KINDS[kind]
    X, y = s.csr()
    eng = _handle(X, y, solver, k, ((groups_key, G), ("relax", 0), ("prb_long", 16),
                                    ("wide", int(kind == "wide"))) + tuple(options))
    _install(eng, s)
    for device in (1, 0):
        eng.set_option("stream_device", device)
        _epoch(eng, solver, k)
        assert eng.get_option(active_key) == 1
        assert eng.get_option("persistent_fallbacks") == 0
        assert eng.get_option(used_key) == device, (kind, device)
        t = eng.debug_stream_tables(kind)
        info = t["info"]
        assert info["device"] == device and info["G"] == G and info["nb"] == s.nb
        assert np.array_equal(t["batch_ptr"], s.batch_ptr) and info["n_entries"] == s.nnz
        if kind == "rowblock":
            assert info["long_thresh"] == 16
            want = host_stream(kind, s, info["G"], long_thresh=info["long_thresh"])
            assert info["has_long"] == int(want["lmask"].any())
        elif kind == "pbcd":
            assert info["NG"] == (16 if k <= 30 else 8)
            assert info["balance"] == dict(options).get("pbprb_balance", 1)
            want = host_stream(kind, s, info["G"], NG=info["NG"], balance=info["balance"])
        else:
            want = host_stream(kind, s, info["G"])
        assert_tables_equal(t, want, (kind, "device" if device else "host"))
    eng.close()
    return want


@pytest.mark.parametrize("name", sorted(STREAM_CASES))
def test_device_rowblock_stream_tables(name):
    s, G = STREAM_CASES[name]
    want = _check_stream("rowblock", s, G)
    if name == "long_slots_31_32_63":   # 16 entries: short; 17: long -- slots 31, 32 and 63
        assert want["lmask"].tolist() == [0, 0x80000001, 0x80000000, 0]
    if name == "more_blocks_than_rows":
        assert not want["lmask"].any()


@pytest.mark.parametrize("name", sorted(STREAM_CASES))
@pytest.mark.parametrize("k,balance", [(5, 1), (40, 0)])
def test_device_pbcd_stream_tables(name, k, balance):
    s, G = STREAM_CASES[name]
    _check_stream("pbcd", s, G, k=k, options=(("pbprb_balance", balance),))


@pytest.mark.parametrize("name", ["group_shapes", "group_shapes_owner_rounds", "tied_groups",
                                  "previous_step_flags"])
@pytest.mark.parametrize("k,balance", [(5, 0), (40, 1)])
def test_device_pbcd_stream_tables_other_group_shapes(name, k, balance):
    s, G = STREAM_CASES[name]
    _check_stream("pbcd", s, G, k=k, options=(("pbprb_balance", balance),))


@pytest.mark.parametrize("name", sorted(WIDE_EDGES))
def test_device_wide_stream_tables(name):
    s, G = WIDE_EDGES[name]
    _check_stream("wide", s, G)


def test_device_relaxed_rowblock_stream_tables():
    """schedule='exact' on a matrix whose neighbouring columns share rows: merged steps, the
    entries on conflict rows left out (device_rowblock_stream with a skip mask)."""
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(400, 80, 10)
    Xc = sp.csc_matrix(X)
    Xc.sort_indices()
    d, k = X.shape[1], 3
    eng = _handle(X, y, "pcd", k, (("wide", 0), ("prb_long", 16), ("prb_groups", 7)))
    eng.set_schedule("exact", np.arange(d, dtype=np.int32))
    for device in (1, 0):
        eng.set_option("stream_device", device)
        eng.set_option("relax", 1)   # (its own invalidation: the merged steps are built again)
        _epoch(eng, "pcd", k)
        assert eng.get_option("relax_steps") > 0 and eng.get_option("persistent_fallbacks") == 0
        t = eng.debug_stream_tables("relaxed")
        info = t["info"]
        assert info["device"] == device and info["G"] == 7 and info["long_thresh"] == 16
        assert info["nb"] == eng.get_option("relax_steps")
        assert sorted(set(t["skip"].tolist())) == [0, 1]
        assert info["n_entries"] == X.nnz - int(t["skip"].sum())
        s = Structure(400, [Xc.indices[Xc.indptr[j]:Xc.indptr[j + 1]] for j in range(d)],
                      [0] + list(range(1, d + 1)))   # (its own steps are not the merged ones)
        want = stream_build_relaxed(s, t)
        assert_tables_equal(t, want, ("relaxed", device))
        assert info["has_long"] == int(want["lmask"].any())
        # the strict stream of the same handle, for cd_linear
        assert eng.get_option("stream_device_used") == device
        strict = eng.debug_stream_tables("rowblock")
        s.batch_ptr = strict["batch_ptr"]
        assert_tables_equal(strict, host_stream("rowblock", s, 7, long_thresh=16), "strict")
    eng.close()


def stream_build_relaxed(s, t):
    """The host entry and the NumPy rule on the merged steps and the skip mask the handle used."""
    s.batch_ptr = t["batch_ptr"]
    want = host_stream("rowblock", s, t["info"]["G"], long_thresh=t["info"]["long_thresh"],
                       skip=t["skip"])
    assert_tables_equal(want, ref_rowblock(s, t["info"]["G"], t["info"]["long_thresh"], t["skip"]))
    return want


# ------------------------------------------------- one epoch pair per stream kind on top
def _two_epochs(kind, s, G, device, k):
    solver = KINDS[kind][0]
    X, y = s.csr()
    eng = _handle(X, y, solver, k, ((KINDS[kind][1], G), ("relax", 0), ("stream_device", device),
                                    ("wide", int(kind == "wide"))))
    _install(eng, s)
    v = [_epoch(eng, solver, k) for _ in range(2)]
    assert eng.get_option(KINDS[kind][2]) == device
    P, w = eng.get_params()
    out = (np.array(v), P, w, eng.get_y_pred())
    eng.close()
    return out


@pytest.mark.parametrize("kind,name,k", [("rowblock", "steps_of_1_33_64", 3),
                                         ("pbcd", "group_shapes", 5), ("wide", "wide_flags", 3)])
def test_epochs_on_device_built_tables_equal_host_built(kind, name, k):
    s, G = (WIDE_EDGES if kind == "wide" else STREAM_CASES)[name]
    dev, host = _two_epochs(kind, s, G, 1, k), _two_epochs(kind, s, G, 0, k)
    for a, b in zip(dev, host):
        assert np.array_equal(a, b)
    assert np.abs(dev[1]).max() > 0


def test_without_the_hook_small_problems_stay_on_the_host_and_keep_nothing():
    s, G = STREAM_CASES["two_steps"]
    X, y = s.csr()
    eng = _handle(X, y, "pcd", 3, (("debug_setup_any_size", 0), ("wide", 0), ("relax", 0)))
    eng.set_schedule("colored", np.arange(s.d, dtype=np.int32))
    assert eng.get_option("colour_device_used") == 0
    with pytest.raises(ValueError, match="has not been built"):
        eng.debug_stream_info("rowblock")
    _epoch(eng, "pcd", 3)
    assert eng.get_option("stream_device_used") == 0
    assert eng.debug_stream_info("rowblock")["device"] == 0
    with pytest.raises(ValueError, match="debug_setup_any_size"):
        eng.debug_stream_tables("rowblock")
    with pytest.raises(ValueError, match="has not been built"):
        eng.debug_stream_info("wide")
    eng.close()


# ----------------------------------------------------------------------------- the colouring
def _colour(n, indptr, indices, order, max_batch, device):
    """(colour_device_used, order, batch_ptr) of the handle's coloured schedule; the engine."""
    d = len(order)
    rng = np.random.RandomState(1)
    X = sp.csc_matrix((rng.randint(1, 4, size=len(indices)).astype(np.float64), indices, indptr),
                      shape=(n, d)).tocsr()
    X.sort_indices()
    wide = int(max_batch > 64)     # classes of more than 64 columns: the wide passes' schedule
    eng = _handle(X, np.ones(n), "pcd", 2,
                  (("colour_device", device), ("max_batch", max_batch), ("wide", wide),
                   ("wide_min_cols", 0), ("prb_groups", 4)))
    o = eng.set_schedule("colored", order)
    sched = eng.get_schedule("colored")
    assert np.array_equal(o, sched.order)
    return eng.get_option("colour_device_used"), sched.order, sched.batch_ptr, eng


def _check_colouring(kind, d, max_batch, shuffled, overflow=False):
    n, indptr, indices = colouring_matrix(kind, d)
    order = visiting_order(d, shuffled)
    cap = min(max_batch, 512 if max_batch > 64 else 64)   # what the persistent passes allow
    want = host_first_fit(n, indptr, indices, order, cap)
    rule = ref_first_fit(n, indptr, indices, order, cap)
    assert np.array_equal(want[0], rule[0]) and np.array_equal(want[1], rule[1])
    for device in (1, 0):
        used, o, bp, eng = _colour(n, indptr, indices, order, max_batch, device)
        assert used == (device if not overflow else 0), (kind, d, max_batch, device)
        assert np.array_equal(o, want[0]) and np.array_equal(bp, want[1])
        if overflow:    # the handle's next calls succeed
            assert np.isfinite(eng.cd_linear_epoch(1.0))
            assert eng.get_option("persistent_fallbacks") == 0
            eng.set_schedule("colored", order)
            assert eng.get_option("colour_device_used") == 0
        eng.close()
    return want


@pytest.mark.parametrize("kind,d,max_batch,shuffled", COLOUR_CASES)
def test_device_first_fit_equals_host_and_rule(kind, d, max_batch, shuffled):
    order, bp = _check_colouring(kind, d, max_batch, shuffled)
    if kind == "shared_row":    # more than 64 colours: the second word of the colour bitmaps
        assert len(bp) - 1 == d
    if kind == "diagonal":      # no conflicts: the classes fill to exactly max_batch, in order
        assert np.array_equal(order, np.arange(d)) and np.diff(bp).max() == min(max_batch, 512)


def test_device_first_fit_4096_colours_and_one_more():
    """4096 pairwise conflicting columns take exactly the 4096 colours of the device's tables;
    with 4097 the device reports the overflow and the host form takes over."""
    order, bp = _check_colouring("shared_row", 4096, 64, False)
    assert len(bp) - 1 == 4096
    order, bp = _check_colouring("shared_row", 4097, 64, False, overflow=True)
    assert len(bp) - 1 == 4097
