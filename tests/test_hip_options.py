"""spfm_set_option / spfm_get_option after the move to one table
(sparsepoly_amd/csrc/spfm_options.inc.h): defaults, ranges and error codes are the parent
commit's, every settable key reads back, and an invalidation rebuilds the same streams, graphs
and relaxed runs.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from test_options_host import engine_rows

pytestmark = pytest.mark.gpu

U = "unknown option"   # spfm_get_option fails with SPFM_ERR_INVALID, "unknown option: <key>"
FREE = "free memory"   # a positive number that depends on the machine

# Recorded on the parent commit (engine tag b4daa878760d, profiles/options_parent_b4daa878760d.json)
# with a fresh handle per key:  key: (get on the fresh handle, [(value set, return code of
# spfm_set_option, get afterwards), ...]) -- the sets of one key are made in this order on one handle.
PARENT = {
    "co_tenants": (1, [(0, -1, 1), (1, 0, 1), (64, 0, 64), (65, -1, 64), (4, 0, 4)]),
    "colour_device": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "colour_device_used": (0, [(0, -1, 0), (1, -1, 0)]),
    "debug_drop_group": (U, [(-2147483648, 0, U), (-1, 0, U), (2, 0, U), (2147483647, 0, U), (0, 0, U)]),
    "debug_keep_last_error": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    # (a test hook added after that record: a plain flag, default 0)
    "debug_setup_any_size": (0, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "debug_spin_max": (U, [(63, -1, U), (64, 0, U), (4096, 0, U), (2147483647, 0, U), (-2147483648, -1, U)]),
    "free_mem_mib": (FREE, [(0, -1, FREE), (1, -1, FREE)]),
    "fuse_chain": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "ingest_device": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "ingest_device_used": (0, [(0, -1, 0), (1, -1, 0)]),
    "interaction_features": (0, [(-1, -1, 0), (0, 0, 0), (3, 0, 3), (2147483647, 0, 2147483647), (-2147483648, -1, 2147483647)]),
    "interaction_launches": (0, [(0, -1, 0), (1, -1, 0)]),
    "interaction_release": (U, [(0, 0, U), (1, 0, U), (-1, 0, U)]),
    "interaction_scratch_kib": (0, [(0, -1, 0), (1, -1, 0)]),
    "interaction_tile_budget": (0, [(-1, -1, 0), (0, 0, 0), (3, 0, 3), (2147483647, 0, 2147483647), (-2147483648, -1, 2147483647)]),
    "max_batch": (4096, [(0, -1, 4096), (1, 0, 1), (512, 0, 512), (2147483647, 0, 2147483647), (-2147483648, -1, 2147483647)]),
    "n_ranks": (1, [(0, -1, 1), (1, -1, 1)]),
    "no_such_option": (U, [(0, -1, U)]),
    "pb_relax_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "pb_stream_device_used": (0, [(0, -1, 0), (1, -1, 0)]),
    "pbcd_fuse": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "pbcd_persistent": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "pbprb_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "pbprb_balance": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "pbprb_dbg": (U, [(-2147483648, 0, U), (-1, 0, U), (0, 0, U), (3, 0, U), (2147483647, 0, U)]),
    "pbprb_groups": (256, [(0, -1, 256), (1, 0, 1), (8, 0, 8), (2147483647, 0, 2147483647), (-2147483648, -1, 2147483647)]),
    "pbprb_owners": (0, [(0, 0, 0), (1, -3, 0), (-1, -3, 0)]),
    "pbprb_stamps": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "pcdw_groups": (0, [(0, -1, 0), (1, 0, 1), (7, 0, 7), (2147483647, 0, 2147483647), (-2147483648, -1, 2147483647)]),
    "pcdw_stamps": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "peer_exchange": (U, [(0, 0, U), (1, -1, U), (-1, -1, U)]),
    "peer_ready": (0, [(0, -1, 0), (1, -1, 0)]),
    "persistent": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "persistent_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "persistent_failed": (0, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "persistent_fallbacks": (0, [(0, -1, 0), (1, -1, 0)]),
    "prb_groups": (64, [(0, -1, 64), (1, 0, 1), (8, 0, 8), (2147483647, 0, 2147483647), (-2147483648, -1, 2147483647)]),
    "prb_lds": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "prb_lds_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "prb_long": (U, [(15, -1, U), (16, 0, U), (100, 0, U), (2147483647, 0, U), (-2147483648, -1, U)]),
    "prb_pack": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "prb_pack_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "prb_stamps": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "probe_lds": (U, [(-2147483648, 0, U), (-1, 0, U), (0, 0, U), (4096, 0, U), (2147483647, 0, U)]),
    "probe_xcd": (U, [(-2147483648, 0, U), (-1, 0, U), (0, 0, U), (5, 0, U), (2147483647, 0, U)]),
    "psgd_eager": (U, [(0, 0, U), (1, 0, U), (2, 0, U), (-1, 0, U)]),
    "psgd_graph_sweeps": (U, [(-1, -1, U), (0, 0, U), (64, 0, U), (65, -1, U), (4, 0, U)]),
    "psgd_redone": (0, [(0, -1, 0), (1, -1, 0)]),
    "relax": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "relax_steps": (0, [(0, -1, 0), (1, -1, 0)]),
    "stream_device": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "stream_device_used": (0, [(0, -1, 0), (1, -1, 0)]),
    "use_graph": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "wide": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "wide_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "wide_ep": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "wide_ep_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "wide_lds_active": (0, [(0, -1, 0), (1, -1, 0)]),
    "wide_lds_rows": (-1, [(-2147483648, 0, -2147483648), (-1, 0, -1), (0, 0, 0), (100, 0, 100), (2147483647, 0, 2147483647)]),
    "wide_min_cols": (110, [(-2147483648, 0, -2147483648), (-1, 0, -1), (0, 0, 0), (64, 0, 64), (2147483647, 0, 2147483647)]),
    "wide_rec8": (1, [(0, 0, 0), (1, 0, 1), (2, 0, 1), (-1, 0, 1)]),
    "wide_stream_device_used": (0, [(0, -1, 0), (1, -1, 0)]),
}

# Keys the parent accepted in spfm_set_option but could not read (U above).  With one table they
# read back: the default below on a fresh handle (the member initialisers of spfm_engine.hip.h),
# then the value last set -- a flag reads 0/1.  The only difference from PARENT that is allowed.
WIDENED = {
    "prb_long": 48, "prb_pack": 1, "prb_stamps": 0, "pcdw_stamps": 0, "pbprb_stamps": 0,
    "pbprb_balance": 1, "pbprb_dbg": 0, "pbcd_fuse": 1, "psgd_eager": 0, "psgd_graph_sweeps": 4,
    "probe_xcd": 0, "probe_lds": 60 * 1024, "debug_spin_max": 1 << 21, "debug_drop_group": 0,
    "debug_keep_last_error": 0, "peer_exchange": 0,
}
FLAGS = {key for key, _, access, _ in engine_rows() if access.startswith("flag(")
         or key == "peer_exchange"}
SETTABLE = [key for key, cls, _, _ in engine_rows() if cls != "READOUT"]


def _engine():
    from sparsepoly_amd.engine import HipEngine

    return HipEngine(0, "f32")


def _get(eng, key):
    v = C.c_int(-12345)
    rc = eng._lib.spfm_get_option(eng._h, key.encode(), C.byref(v))
    if rc != 0:
        assert rc == -1 and eng._lib.spfm_last_error(eng._h).decode() == "unknown option: " + key
        return U
    return v.value


def _same(got, want):
    return got > 0 if want == FREE else got == want


def test_parent_table_covers_every_key():
    assert set(PARENT) - {"no_such_option"} == {r[0] for r in engine_rows()}
    assert set(WIDENED) == {k for k, (g, _) in PARENT.items()
                            if g == U and k not in ("no_such_option", "interaction_release")}


def test_defaults_ranges_and_error_codes_are_the_parents():
    seen = []
    for key, (fresh, sets) in sorted(PARENT.items()):
        eng = _engine()
        cur = WIDENED.get(key)
        got = _get(eng, key)
        seen.append((key, "get", got))
        assert _same(got, fresh if cur is None else cur), (key, got, fresh, cur)
        for value, rc, after in sets:
            got_rc = eng._lib.spfm_set_option(eng._h, key.encode(), value)
            msg = eng._lib.spfm_last_error(eng._h).decode()
            got = _get(eng, key)
            seen.append((key, value, got_rc, got))
            assert got_rc == rc, (key, value, got_rc, rc, msg)
            if key not in SETTABLE:   # a read-out, or no key at all
                assert rc == -1 and msg == "unknown option: " + key, (key, msg)
            if key in ("pbprb_owners", "peer_exchange") and rc != 0:
                assert msg.startswith(key + ": "), msg
            if cur is not None:   # formerly write-only: reads back the value last set
                if rc == 0:
                    cur = int(value != 0) if key in FLAGS else value
                after = cur
            assert _same(got, after), (key, value, got, after)
        eng.close()
    print(seen)


def test_unknown_key_fails_the_same_way_from_both_functions():
    eng = _engine()
    with pytest.raises(ValueError, match=r"^unknown option: no_such_option$"):
        eng.set_option("no_such_option", 1)
    with pytest.raises(ValueError, match=r"^unknown option: no_such_option$"):
        eng.get_option("no_such_option")
    with pytest.raises(NotImplementedError):
        eng.set_option("pbprb_owners", 1)
    eng.close()


# one in-range value per key that differs from the default where the key allows one
_ROUND_TRIP = {"max_batch": 512, "prb_groups": 8, "prb_long": 100, "pbprb_groups": 8,
               "pbprb_owners": 0, "wide_min_cols": 64, "pcdw_groups": 7, "wide_lds_rows": 100,
               "co_tenants": 4, "peer_exchange": 0, "psgd_graph_sweeps": 9,
               "interaction_tile_budget": 3, "interaction_features": 5, "pbprb_dbg": 3,
               "probe_xcd": 5, "probe_lds": 4096, "debug_spin_max": 4096, "debug_drop_group": 2}


@pytest.mark.parametrize("key", SETTABLE)
def test_set_then_get_round_trips(key):
    eng = _engine()
    if key == "interaction_release":   # an action: nothing to read
        eng.set_option(key, 0)
        assert _get(eng, key) == U
    elif key in FLAGS and key not in _ROUND_TRIP:
        first = eng.get_option(key)
        for value in (1 - first, first):
            eng.set_option(key, value)
            assert eng.get_option(key) == value
    else:
        eng.set_option(key, _ROUND_TRIP[key])
        assert eng.get_option(key) == _ROUND_TRIP[key]
    eng.close()


def test_co_tenants_caps_the_workgroup_counts():
    cus = 256   # compute units of an MI355X
    eng = _engine()
    assert eng.device_name.startswith("gfx950")
    defaults = {k: eng.get_option(k) for k in ("prb_groups", "pbprb_groups")}
    assert defaults == {"prb_groups": 64, "pbprb_groups": 256}
    eng.set_option("co_tenants", 4)
    for k, v in defaults.items():
        assert eng.get_option(k) == min(v, cus // 4), k
    assert eng.get_option("pcdw_groups") == 0   # the wide pass caps itself
    eng.close()


# ---------------------------------------------------------------- invalidation leaves results alone
N, D, K, EPOCHS = 300, 40, 3, 3
# tuning keys with a non-empty invalidation mask, from the engine's table
_MASKED_TUNING = [key for key, cls, _, mask in engine_rows() if cls == "TUNING" and mask != "0"]


def _problem():
    rng = np.random.RandomState(5)
    X = sp.random(N, D, density=8.0 / D, random_state=rng, data_rvs=rng.randn, format="csr")
    X.data = X.data.astype(np.float32).astype(np.float64)
    return X, rng.randn(N).astype(np.float32).astype(np.float64)


def _reset_every_masked_key(eng):
    """Sets every such key to the value it has.  peer_exchange comes first: it asks for the
    schedule again.  pcdw_groups reads 0 (= not chosen yet) while no wide stream exists, which
    is outside its range [1, ..]: nothing to write back then."""
    keys = ["peer_exchange"] + [k for k in _MASKED_TUNING if k != "peer_exchange"]
    for key in keys:
        value = eng.get_option(key)
        if key == "pcdw_groups" and value == 0:
            continue
        eng.set_option(key, value)
        assert eng.get_option(key) == value
        if key == "peer_exchange":
            eng.set_schedule("colored", np.arange(D, dtype=np.int32))


def _fit(solver, reg, between=None):
    X, y = _problem()
    eng = _engine()
    eng.set_data(X, y)
    eng.set_params(0.05 * np.random.RandomState(1).randn(1, K, D), np.zeros(D),
                   np.where(np.arange(K) % 2 == 0, 1.0, -1.0))
    eng.configure(solver, "squared", reg, 2)
    eng.init_pred(2, True, False)
    eng.set_schedule("colored", np.arange(D, dtype=np.int32))
    ic = np.arange(K, dtype=np.int32)
    for epoch in range(EPOCHS):
        eng.cd_linear_epoch(0.5)
        if solver == "pcd":
            eng.pcd_epoch(0, 2, 10.0, 1e-3, 1.0, ic)
        else:
            eng.pbcd_epoch(0, 2, 1.0, 1e-3, 1.0)
        if between is not None and epoch + 1 < EPOCHS:
            between(eng, epoch)
    P, w = eng.get_params()
    out = dict(P=P.copy(), w=w.copy(), y_pred=eng.get_y_pred().copy(),
               fallbacks=eng.get_option("persistent_fallbacks"))
    eng.close()
    return out


def _assert_bit_equal(a, b):
    assert a["fallbacks"] == 0 and b["fallbacks"] == 0
    for name in ("P", "w", "y_pred"):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert np.abs(a["P"]).max() > 0


@pytest.mark.parametrize("solver,reg", [("pcd", "squaredl12"), ("pbcd", "omegacs")])
def test_invalidation_leaves_results_alone(solver, reg):
    assert len(_MASKED_TUNING) >= 25 and "prb_groups" in _MASKED_TUNING
    a = _fit(solver, reg)
    b = _fit(solver, reg, between=lambda eng, epoch: _reset_every_masked_key(eng))
    _assert_bit_equal(a, b)

    # another workgroup count sums the partials of the 64-column pass in another order: compare
    # two runs that make the same two changes at the same epochs
    def groups(eng, epoch):
        eng.set_option("prb_groups", 8 if epoch == 0 else 64)

    _assert_bit_equal(_fit(solver, reg, between=groups), _fit(solver, reg, between=groups))
