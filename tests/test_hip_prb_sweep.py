"""The granule sweep of the persistent 64-column passes (prb_collect_quarter in pcd_prb_kernel and
lin_prb_kernel): a wave whose part of the workgroup range is a whole number of groups of eight
(prb_groups a multiple of 64) sweeps it in a straight line -- one address per lane, the tags tested
on the low words, one retry decision per wave -- every other part length runs the general code.
Both must form the same sums in the same order.

1. The probe (HipEngine.debug_sweep_sums: one workgroup runs the passes' own sweep over values the
   caller gives) against a NumPy reference, BITWISE.  The contract: a value loses its two lowest
   mantissa bits (they carry the step's tag), a part's workgroups are added in ascending order
   starting from 0.0, then the eight part sums in ascending order; all in float64.
2. The small fit of tests/test_hip_prb_records.py at part lengths 0/1 (3 row blocks), 5 (40),
   8 (64: the straight-line sweep) and 9 (72): rows in LDS against rows in global memory bitwise,
   the LDS form against the CPU oracle at the f32 tolerances of tests/test_hip_parity.py.
3. The NumPy reference itself against plain Python addition (no GPU).

GPU tests need a real MI355X: ``pytest -m gpu``."""
import struct

import numpy as np
import pytest
import scipy.sparse as sp

P_ATOL = 1e-4      # tests/test_hip_parity.py, precision='f32'
TRAJ_RTOL = 1e-5
PRED_ATOL = 2e-4

PARTS = 8          # kPrbParts: sweeping waves of a workgroup
K = 3
EPOCHS = 2

GROUPS = [1, 3, 8, 40, 64, 72, 128]
NCOLS = [1, 37, 64]
STEPS = [0, 1, 2, 5]   # tags 1, 1, 2, 3; both slab parities


def clear_tag_bits(vals):
    v = np.ascontiguousarray(vals, dtype=np.float64)
    return (v.view(np.int64) & np.int64(~3)).view(np.float64)


def sweep_reference(vals, ncols):
    """vals[groups, 64, nv] -> totals [64, nv] in the sweep's order of summation."""
    v = clear_tag_bits(vals)
    groups = v.shape[0]
    total = None
    for w in range(PARTS):
        g0, g1 = groups * w // PARTS, groups * (w + 1) // PARTS
        part = np.zeros(v.shape[1:], dtype=np.float64)
        for g in range(g0, g1):
            part = part + v[g]
        total = part if total is None else total + part
    total[ncols:] = 0.0
    return total


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _values(kind, groups, nv, seed):
    rng = np.random.RandomState(seed)
    shape = (groups, 64, nv)
    if kind == "zeros":
        return np.zeros(shape)
    v = rng.randn(*shape) * 10.0 ** rng.uniform(-8, 8, shape)
    if kind == "signed-zeros":
        z = rng.rand(*shape)
        v = np.where(z < 0.25, 0.0, np.where(z < 0.5, -0.0, v))
    return v


def test_reference_is_plain_sequential_addition():
    """The yardstick of the probe test on a 3 x 64 x 2 example, against Python floats added one
    by one: 3 row blocks over 8 parts are the parts [], [], [0], [], [], [1], [], [2]."""
    vals = _values("random", 3, 2, seed=11)
    vals[1, 5, 0] = -0.0
    ref = sweep_reference(vals, 37)
    bounds = [(3 * w // 8, 3 * (w + 1) // 8) for w in range(8)]
    assert bounds == [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 3)]

    def cleared(x):
        (u,) = struct.unpack("<Q", struct.pack("<d", x))
        return struct.unpack("<d", struct.pack("<Q", u & ~3))[0]

    for q in range(64):
        for v in range(2):
            tot = None
            for g0, g1 in bounds:
                part = 0.0
                for g in range(g0, g1):
                    part = part + cleared(float(vals[g, q, v]))
                tot = part if tot is None else tot + part
            if q >= 37:
                tot = 0.0
            assert struct.pack("<d", tot) == struct.pack("<d", float(ref[q, v])), (q, v)
    # the two lowest mantissa bits are really dropped: 1 + 3 ulp -> 1
    one = np.full((1, 64, 1), np.nextafter(np.nextafter(np.nextafter(1.0, 2), 2), 2))
    assert (sweep_reference(one, 64) == 1.0).all()


@pytest.fixture(scope="module")
def engine():
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f32")
    yield eng
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("groups", GROUPS)
def test_probe_sums_bitwise(engine, groups):
    """64 and 128 row blocks: one and two groups of eight per part (straight-line sweep); 72: a part
    of nine; 40: five; 1 and 3: empty parts."""
    for nv in (1, 2):
        for kind in ("random", "zeros", "signed-zeros"):
            vals = _values(kind, groups, nv, seed=100 * groups + nv)
            for ncols in NCOLS:
                for step in STEPS:
                    got = engine.debug_sweep_sums(vals, ncols=ncols, step=step)
                    ref = sweep_reference(vals, ncols)
                    assert got.shape == (64, nv)
                    np.testing.assert_array_equal(
                        _bits(got), _bits(ref),
                        err_msg="groups %d nv %d %s ncols %d step %d" % (groups, nv, kind, ncols,
                                                                        step))
                    assert (_bits(got[ncols:]) == 0).all()


# ---- the small fit -------------------------------------------------------------------------
CONFIGS = {  # loss, regularizer, LDS form
    "fm2-squared": ("squared", "squaredl12", 1),
    "fm2-logistic": ("logistic", "omegati", 2),
}
N, D, PER_ROW = 2000, 300, 12


def _problem(loss):
    rng = np.random.RandomState(7)
    cols = np.stack([rng.choice(D, PER_ROW, replace=False) for _ in range(N)])
    vals = rng.randn(N, PER_ROW).astype(np.float32).astype(np.float64)
    X = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, PER_ROW * N + 1, PER_ROW)),
                      shape=(N, D))
    X.sort_indices()
    # squared loss: y = 0, so that the LDS residual word equals yhat bit for bit
    # (tests/test_hip_prb_records.py, module docstring)
    y = np.zeros(N) if loss == "squared" else np.where(
        np.random.RandomState(5).randn(N) > 0, 1.0, -1.0)
    return X, y


def _run(X, y, config, lds, groups, schedule):
    from sparsepoly_amd.engine import HipEngine

    loss, reg, _ = CONFIGS[config]
    Xc = X.tocsc()
    Xc.sort_indices()
    eng = HipEngine(0, "f32")
    eng.set_option("prb_groups", groups)
    eng.set_option("prb_lds", lds)
    eng.set_data(Xc, y)
    P0 = 0.2 * np.random.RandomState(0).randn(1, K, D)
    lams = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    eng.set_params(P0, np.zeros(D), lams)
    eng.configure("pcd", loss, reg, 2)
    eng.init_pred(2, True, False)
    order = eng.set_schedule(schedule, np.arange(D, dtype=np.int32))
    ic = np.arange(K, dtype=np.int32)
    viol = []
    for _ in range(EPOCHS):
        v = eng.cd_linear_epoch(0.5)
        v += eng.pcd_epoch(0, 2, 10.0, 1e-3, 0.1, ic)
        viol.append(v)
    P, w = eng.get_params()
    out = dict(viol=np.array(viol), P=P, w=w, y_pred=eng.get_y_pred(), order=order, P0=P0,
               lams=lams, lds=eng.get_option("prb_lds_active"),
               relaxed=eng.get_option("relax_steps"),
               fallbacks=eng.get_option("persistent_fallbacks"))
    eng.close()
    return out


_ORACLE_FITS = {}


def _oracle_fit(oracle, X, y, config, r):
    """One CPU fit per (configuration, visiting order), shared by the cases that report it."""
    loss, reg, _ = CONFIGS[config]
    key = (config, r["order"].tobytes())
    if key not in _ORACLE_FITS:
        fm = oracle.OracleFM(degree=2, loss=loss, n_components=K, solver="pcd", regularizer=reg,
                             alpha=0.5, beta=10.0, gamma=1e-3, eta0=0.1, tol=0, max_iter=EPOCHS,
                             fit_linear=True, feature_order=r["order"])
        fm.fit(X, y, P_init=r["P0"], lams_init=r["lams"])
        _ORACLE_FITS[key] = fm
    return _ORACLE_FITS[key]


def _check(oracle, config, groups, schedule="colored"):
    loss, _, mode = CONFIGS[config]
    X, y = _problem(loss)
    r = _run(X, y, config, 1, groups, schedule)
    g = _run(X, y, config, 0, groups, schedule)
    assert r["lds"] == mode and g["lds"] == 0
    assert r["fallbacks"] == 0 and g["fallbacks"] == 0
    np.testing.assert_array_equal(r["order"], g["order"])
    for name in ("viol", "P", "w", "y_pred"):
        np.testing.assert_array_equal(_bits(r[name]), _bits(g[name]), err_msg=name)
    fm = _oracle_fit(oracle, X, y, config, r)
    np.testing.assert_allclose(r["viol"], [h[0] for h in fm.history], rtol=TRAJ_RTOL)
    np.testing.assert_allclose(r["P"].reshape(fm.P_.shape), fm.P_, rtol=0, atol=P_ATOL)
    np.testing.assert_allclose(r["w"], fm.w_, rtol=0, atol=P_ATOL)
    np.testing.assert_allclose(r["y_pred"], fm.y_pred_, rtol=0, atol=PRED_ATOL)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [3, 40, 64, 72])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fit_at_every_part_length(oracle, config, groups):
    _check(oracle, config, groups)


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_exact_schedule_runs_the_relaxed_instantiation(oracle, config):
    """The reference's own order: columns that share rows are merged into relaxed steps, whose
    kernels (CR instantiations) call the same sweep; 64 row blocks = the straight-line sweep."""
    r = _check(oracle, config, 64, schedule="exact")
    assert r["relaxed"] > 0
