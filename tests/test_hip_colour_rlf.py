"""The RLF colouring on the device (csrc/spfm_colour.hip, device_rlf) against the host form
(csrc/spfm_schedule.cpp, schedule_rlf): the same order and the same batch boundaries; fits in the
new order against the oracle replaying that order; a saved Schedule.  The matrices are small, so
SPFM_RLF_DEVICE=1 lifts the device form's size threshold (one case is above the threshold and
needs no hint)."""
import json
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import golden_csr, load_golden

from test_hip_parity import P_ATOL, TRAJ_RTOL, _Run

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_form_at_any_size(monkeypatch):
    monkeypatch.setenv("SPFM_RLF_DEVICE", "1")


def _matrix(n, d, per_row, seed, zipf=False, empty=False):
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), per_row)
    if zipf:
        p = 1.0 / np.arange(1, d + 1) ** 0.9
        cols = rng.choice(d, size=n * per_row, p=p / p.sum())
    else:
        cols = rng.randint(0, d, size=n * per_row)
    X = sp.csr_matrix((rng.randn(n * per_row), (rows, cols)), shape=(n, d))
    X.sum_duplicates()
    if empty:
        keep = np.ones(d)
        keep[[0, 1, d // 2, d - 1]] = 0
        X = sp.csr_matrix(X @ sp.diags(keep))
        X.eliminate_zeros()
    X.sort_indices()
    return X


def _private_rows(d, per_col):
    idx = np.arange(d * per_col, dtype=np.int32)
    X = sp.csc_matrix((np.ones(d * per_col), idx, per_col * np.arange(d + 1, dtype=np.int64)),
                      shape=(d * per_col, d))
    return X.tocsr()


def _schedule(X, device, order, solver="pcd", degree=2, options=()):
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f32")
    eng.set_option("colour_device", device)
    for key, v in options:
        eng.set_option(key, v)
    n, d = X.shape
    eng.set_data(X, np.random.RandomState(9).randn(n))
    eng.set_params(0.01 * np.random.RandomState(0).randn(degree - 1, 3, d), np.zeros(d), np.ones(3))
    eng.configure(solver, "squared", "l1", degree)
    eng.init_pred(degree, True, degree > 2)
    o = eng.set_schedule("colored_rlf", order)
    used = eng.get_option("colour_device_used")
    bp = eng.get_schedule("colored_rlf").batch_ptr
    eng.close()
    return used, o, bp


def _shuffled(d, seed=4):
    o = np.arange(d, dtype=np.int32)
    np.random.RandomState(seed).shuffle(o)
    return o


CASES = {
    # name: (matrix, visiting order or None, solver, degree, options, widths expected or None)
    "odd_d": (lambda: _matrix(3000, 333, 4, 1), None, "pcd", 3, (), None),
    "empty_columns": (lambda: _matrix(2000, 300, 4, 2, empty=True), None, "pcd", 3, (), None),
    "zipf_long_columns": (lambda: _matrix(4000, 150, 5, 3, zipf=True), None, "pbcd", 2, (), None),
    "cap_64_reached": (lambda: _private_rows(200, 3), None, "pcd", 2, (("wide", 0),),
                       [64, 64, 64, 8]),
    "cap_512_wide_classes": (lambda: _matrix(1500, 1300, 3, 5), None, "pcd", 2,
                             (("wide_min_cols", 0),), None),
    "cap_512_reached": (lambda: _private_rows(700, 2), None, "pcd", 2, (("wide_min_cols", 0),),
                        [512, 188]),
    "recoloured_with_64": (lambda: _matrix(1500, 400, 3, 6), None, "pcd", 2, (), None),
    "shuffled": (lambda: _matrix(3000, 333, 4, 1), _shuffled(333), "pcd", 3, (), None),
    "fewer_columns_than_a_wave": (lambda: _matrix(100, 9, 2, 7), None, "pcd", 3, (), None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_form_equals_host_form(name):
    make, order, solver, degree, options, widths = CASES[name]
    X = make()
    d = X.shape[1]
    if order is None:
        order = np.arange(d, dtype=np.int32)
    dev = _schedule(X, 1, order, solver, degree, options)
    host = _schedule(X, 0, order, solver, degree, options)
    assert dev[0] == 1 and host[0] == 0
    assert np.array_equal(dev[2], host[2])          # the batch boundaries
    assert np.array_equal(dev[1], host[1])          # the order
    assert sorted(dev[1].tolist()) == list(range(d))
    got = np.diff(dev[2])
    if widths is not None:
        assert got.tolist() == widths
    if name == "cap_512_wide_classes":
        assert got.max() > 64
    if name == "zipf_long_columns":
        assert np.diff(X.tocsc().indptr).max() > 64
    Xc = X.tocsc()
    for b in range(len(dev[2]) - 1):
        cols = dev[1][dev[2][b]:dev[2][b + 1]]
        rows = np.concatenate([Xc.indices[Xc.indptr[j]:Xc.indptr[j + 1]] for j in cols])
        assert len(rows) == len(np.unique(rows))


def test_above_the_size_threshold_without_the_hint(monkeypatch):
    monkeypatch.delenv("SPFM_RLF_DEVICE")
    X = _matrix(30000, 5000, 40, 11)
    assert X.nnz >= (1 << 20)
    order = np.arange(5000, dtype=np.int32)
    dev = _schedule(X, 1, order, "pcd", 3)
    host = _schedule(X, 0, order, "pcd", 3)
    assert dev[0] == 1 and host[0] == 0
    assert np.array_equal(dev[2], host[2]) and np.array_equal(dev[1], host[1])
    small = _schedule(_matrix(3000, 333, 4, 1), 1, np.arange(333, dtype=np.int32), "pcd", 3)
    assert small[0] == 0                            # below the threshold: the host form


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("case", ["c2|squared", "c3|squared", "c4|squared", "c4d3|logistic"])
def test_fit_equals_oracle_in_the_reported_order(oracle, case, precision):
    """pcd degree 2 and 3, pbcd, and the cd_linear epoch of each, in the RLF order"""
    z = load_golden("g3_small_configs.npz")
    X = golden_csr(z)
    meta = json.loads(str(z["meta|" + case]))
    y = z["y"]
    if meta["loss"] != "squared":
        y = np.where(y > np.median(y), 1.0, -1.0)
    r = _Run(X, y, meta, z["P0|" + case], z["lams|" + case], precision, schedule="colored_rlf")
    assert sorted(r.order) == list(range(X.shape[1]))
    fm = oracle.OracleFM(degree=meta["degree"], loss=meta["loss"], n_components=meta["k"],
                         solver=meta["solver"], regularizer=meta["regularizer"],
                         alpha=meta["alpha"], beta=meta["beta"], gamma=meta["gamma"], tol=0,
                         fit_lower="explicit", fit_linear=True, max_iter=4,
                         feature_order=r.order)
    fm.fit(X, y, P_init=z["P0|" + case], lams_init=z["lams|" + case])
    np.testing.assert_allclose(r.viol, [h[0] for h in fm.history], rtol=TRAJ_RTOL[precision])
    np.testing.assert_allclose(r.loss, [h[1] for h in fm.history], rtol=TRAJ_RTOL[precision])
    np.testing.assert_allclose(r.P, fm.P_, rtol=0, atol=P_ATOL[precision])
    np.testing.assert_allclose(r.w, fm.w_, rtol=0, atol=P_ATOL[precision])


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_wide_pass_in_the_rlf_order_equals_oracle(oracle, precision):
    """classes of more than 64 columns: the wide passes (degree-2 pcd, cd_linear) run them"""
    from sparsepoly_amd.engine import HipEngine

    X = _matrix(1500, 1300, 3, 5)
    X.data = X.data.astype(np.float32).astype(np.float64)
    n, d = X.shape
    k = 3
    rng = np.random.RandomState(8)
    y = rng.randn(n).astype(np.float32).astype(np.float64)
    P0 = 0.01 * rng.randn(1, k, d)
    lams = np.ones(k)
    alpha, beta, gamma = 0.1, 1.0, 1e-3
    eng = HipEngine(0, precision)
    eng.set_option("wide_min_cols", 0)
    eng.set_data(X, y)
    eng.set_params(P0, np.zeros(d), lams)
    eng.configure("pcd", "squared", "l1", 2)
    eng.init_pred(2, False, False)
    order = eng.set_schedule("colored_rlf", np.arange(d, dtype=np.int32))
    assert eng.get_option("colour_device_used") == 1 and eng.get_option("wide_active") == 1
    assert np.diff(eng.get_schedule("colored_rlf").batch_ptr).max() > 64
    viol, loss = [], []
    for _ in range(4):
        v = eng.cd_linear_epoch(alpha)
        v += eng.pcd_epoch(0, 2, beta, gamma, 1.0, np.arange(k, dtype=np.int32))
        viol.append(v)
        loss.append(eng.loss_sum())
    P, w = eng.get_params()
    eng.close()
    fm = oracle.OracleFM(degree=2, loss="squared", n_components=k, solver="pcd", regularizer="l1",
                         alpha=alpha, beta=beta, gamma=gamma, tol=0, fit_lower="explicit",
                         fit_linear=True, max_iter=4, feature_order=order)
    fm.fit(X, y, P_init=P0, lams_init=lams)
    np.testing.assert_allclose(viol, [h[0] for h in fm.history], rtol=TRAJ_RTOL[precision])
    np.testing.assert_allclose(loss, [h[1] for h in fm.history], rtol=TRAJ_RTOL[precision])
    np.testing.assert_allclose(P, fm.P_, rtol=0, atol=P_ATOL[precision])
    np.testing.assert_allclose(w, fm.w_, rtol=0, atol=P_ATOL[precision])


def test_saved_schedule_gives_the_same_fit(tmp_path):
    from sparsepoly_amd import SparseFactorizationMachineRegressor
    from sparsepoly_amd.schedule import Schedule

    X = _matrix(600, 90, 4, 12)
    X.data = X.data.astype(np.float32).astype(np.float64)
    y = np.random.RandomState(13).randn(600).astype(np.float32).astype(np.float64)
    kw = dict(degree=3, n_components=4, solver="pcd", regularizer="l1", alpha=0.1, beta=1.0,
              gamma=1e-3, max_iter=3, tol=0, random_state=0, device=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = SparseFactorizationMachineRegressor(schedule="colored_rlf", **kw).fit(X, y)
        Schedule.build(X, "colored_rlf").save(str(tmp_path / "rlf.npz"))
        s = Schedule.load(str(tmp_path / "rlf.npz"))
        assert s.mode == "colored_rlf"
        b = SparseFactorizationMachineRegressor(schedule=s, **kw).fit(X, y)
    assert np.array_equal(a.feature_order_, s.order)
    assert np.array_equal(a.schedule_.batch_ptr, s.batch_ptr)
    assert a.n_steps_per_sweep_ == b.n_steps_per_sweep_ == s.n_batches
    np.testing.assert_array_equal(a.P_, b.P_)
    np.testing.assert_array_equal(a.w_, b.w_)
