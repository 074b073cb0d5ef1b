"""The LDS image of a row block in the persistent 64-column passes (pcd_prb_kernel,
lin_prb_kernel): filled at the start and written back at the end of every launch, eight trips'
loads in flight at a time.  A block that fills the LDS (15 625 rows, the flagship's block
shape: 31 trips per thread), blocks whose last batch of trips is partial, and a block with
fewer rows than threads -- against the same passes with the rows in global memory and against
the CPU oracle in the engine's reported order, at the f32 tolerances of
tests/test_hip_parity.py.  Needs a real MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

P_ATOL = 1e-4      # tests/test_hip_parity.py, precision='f32'
TRAJ_RTOL = 1e-5


def _problem(n, d=300, per_row=3, seed=3):
    rng = np.random.RandomState(seed)
    cols = np.stack([rng.choice(d, per_row, replace=False) for _ in range(n)])
    vals = rng.randn(n, per_row).astype(np.float32).astype(np.float64)
    X = sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(0, per_row * n + 1, per_row)),
                      shape=(n, d))
    X.sort_indices()
    y = rng.randn(n).astype(np.float32).astype(np.float64)
    return X, y


def _run(X, y, loss, reg, lds, k=3, epochs=2):
    from sparsepoly_amd.engine import HipEngine

    d = X.shape[1]
    Xc = X.tocsc()
    Xc.sort_indices()
    eng = HipEngine(0, "f32")
    eng.set_option("prb_groups", 2)
    eng.set_option("prb_lds", lds)
    eng.set_data(Xc, y)
    P0 = 0.01 * np.random.RandomState(0).randn(1, k, d)
    eng.set_params(P0, np.zeros(d), np.ones(k))
    eng.configure("pcd", loss, reg, 2)
    eng.init_pred(2, True, False)
    order = eng.set_schedule("colored", np.arange(d, dtype=np.int32))
    ic = np.arange(k, dtype=np.int32)
    viol = [eng.cd_linear_epoch(0.5) + eng.pcd_epoch(0, 2, 10.0, 1e-3, 1.0, ic)
            for _ in range(epochs)]
    P, w = eng.get_params()
    out = dict(viol=np.array(viol), P=P, w=w, y_pred=eng.get_y_pred(), order=order, P0=P0,
               lds=eng.get_option("prb_lds_active"),
               fallbacks=eng.get_option("persistent_fallbacks"))
    eng.close()
    return out


# rows, loss, regularizer, LDS form: 2 x 15 625 rows = the LDS full, 31 trips per thread;
# 2 x 15 007 rows (+-1 targets: prediction word + sign byte): the last eight trips partial;
# 2 x 2 350 rows: one partial batch of trips; 2 x 175 rows: threads without any row
CASES = [(31_250, "squared", "squaredl12", 1), (30_013, "logistic", "l1", 2),
         (4_700, "squared", "squaredl12", 1), (350, "logistic", "squaredl12", 2)]


@pytest.mark.parametrize("n,loss,reg,mode", CASES)
def test_lds_image_fill_and_write_back(oracle, n, loss, reg, mode):
    X, y = _problem(n)
    if loss != "squared":
        y = np.where(y > np.median(y), 1.0, -1.0)
    r = _run(X, y, loss, reg, 1)
    g = _run(X, y, loss, reg, 0)
    assert r["lds"] == mode and g["lds"] == 0
    assert r["fallbacks"] == 0 and g["fallbacks"] == 0
    np.testing.assert_array_equal(r["order"], g["order"])
    # the two forms round differently (residual vs prediction in float); each is held to the
    # oracle within TRAJ_RTOL / P_ATOL below, so they differ by at most twice that
    np.testing.assert_allclose(r["viol"], g["viol"], rtol=2 * TRAJ_RTOL)
    np.testing.assert_allclose(r["P"], g["P"], rtol=0, atol=2 * P_ATOL)
    np.testing.assert_allclose(r["w"], g["w"], rtol=0, atol=2 * P_ATOL)
    np.testing.assert_allclose(r["y_pred"], g["y_pred"], rtol=0, atol=2e-3)
    fm = oracle.OracleFM(degree=2, loss=loss, n_components=3, solver="pcd", regularizer=reg,
                         alpha=0.5, beta=10.0, gamma=1e-3, tol=0, max_iter=2, fit_linear=True,
                         feature_order=r["order"])
    fm.fit(X, y, P_init=r["P0"], lams_init=np.ones(3))
    np.testing.assert_allclose(r["viol"], [h[0] for h in fm.history], rtol=TRAJ_RTOL)
    np.testing.assert_allclose(r["P"], fm.P_, rtol=0, atol=P_ATOL)
    np.testing.assert_allclose(r["w"], fm.w_, rtol=0, atol=P_ATOL)
    np.testing.assert_allclose(r["y_pred"], fm.y_pred_, rtol=0, atol=1e-3)
