"""sparsepoly_amd.kernels on the device (spfm_gram_csr_dense / spfm_gram_csr_csr) against the
reference-generated goldens (g6 anova_kernel / poly_predict, g8 all_subsets_kernel), brute force,
the NumPy restatement of kernels.py in oracle/ and the estimators' validated predict path.
Needs a real MI355X: ``pytest -m gpu``."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _km():
    from sparsepoly_amd import kernels

    return kernels


def _dp(Xd, Pd, kind, degree):
    """Float64 restatement on the host: the products x_c p_c of every pair, in feature order."""
    n1, n2 = Xd.shape[0], Pd.shape[0]
    if kind == "poly":
        return (Xd @ Pd.T) ** degree
    if kind == "all-subsets":
        K = np.ones((n1, n2))
        for c in range(Xd.shape[1]):
            K *= 1 + np.outer(Xd[:, c], Pd[:, c])
        return K
    m = max(degree, 1)
    a = [np.ones((n1, n2))] + [np.zeros((n1, n2)) for _ in range(m)]
    for c in range(Xd.shape[1]):
        v = np.outer(Xd[:, c], Pd[:, c])
        for t in range(m, 0, -1):
            a[t] = a[t] + a[t - 1] * v
    return a[m]


def _brute_anova(Xd, Pd, m):
    n1, n2, d = Xd.shape[0], Pd.shape[0], Xd.shape[1]
    K = np.zeros((n1, n2))
    for comb in itertools.combinations(range(d), m):
        c = list(comb)
        K += np.prod(Xd[:, None, c] * Pd[None, :, c], axis=2)
    return K


def _sparse_x(n, d, density, seed):
    rng = np.random.RandomState(seed)
    X = sp.random(n, d, density=density, format="csr", random_state=rng, data_rvs=rng.randn)
    return X


# ------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("m", [2, 3, 4, 5])
def test_anova_and_poly_predict_match_reference_goldens(m):
    km = _km()
    z = load_golden("g6_anova.npz")
    Xd, P, lams = z["X"], z["P"], z["lams"]
    for X, key in ((Xd, "K_dense|deg%d" % m), (sp.csr_matrix(Xd), "K_sparse|deg%d" % m)):
        K = km.anova_kernel(X, P, m)
        assert isinstance(K, np.ndarray) and K.shape == z[key].shape
        scale = max(1.0, float(np.abs(z[key]).max()))
        np.testing.assert_allclose(K, z[key], rtol=0, atol=1e-10 * scale)
    ref = z["pred|deg%d" % m]
    pred = km.poly_predict(Xd, P, lams, kernel="anova", degree=m)
    assert pred.shape == ref.shape
    np.testing.assert_allclose(pred, ref, rtol=0, atol=1e-10 * max(1.0, float(np.abs(ref).max())))


def test_all_subsets_matches_reference_golden():
    km = _km()
    z = load_golden("g8_all_subsets.npz")
    for X in (z["X"], sp.csr_matrix(z["X"])):
        K = km.all_subsets_kernel(X, z["P_true"])
        np.testing.assert_allclose(K, z["K"], rtol=0, atol=1e-10 * float(np.abs(z["K"]).max()))
        pred = km.poly_predict(X, z["P_true"], z["lams_true"], "all-subsets")
        np.testing.assert_allclose(pred, z["K"] @ z["lams_true"], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ 2. operand forms
def _awkward_pair(seed=3):
    """X with an empty row, a row with no feature in common with P, and P with an empty row."""
    rng = np.random.RandomState(seed)
    d = 12
    Xd = rng.randn(9, d) * (rng.rand(9, d) < 0.5)
    Pd = rng.randn(7, d) * (rng.rand(7, d) < 0.6)
    Xd[2] = 0.0
    Pd[4] = 0.0
    Pd[:, :3] = 0.0
    Xd[5] = 0.0
    Xd[5, :3] = rng.randn(3)  # only features P never uses
    return Xd, Pd


@pytest.mark.parametrize("kind,degree", [("anova", 1), ("anova", 2), ("anova", 3), ("anova", 5),
                                         ("poly", 2), ("poly", 3), ("all-subsets", 0)])
def test_four_operand_forms_agree(kind, degree):
    km = _km()
    Xd, Pd = _awkward_pair()
    f = {"anova": lambda A, B: km.anova_kernel(A, B, degree),
         "poly": lambda A, B: km.homogeneous_kernel(A, B, degree),
         "all-subsets": lambda A, B: km.all_subsets_kernel(A, B)}[kind]
    ref = _dp(Xd, Pd, kind, degree)
    Ks = [f(A, B) for A in (Xd, sp.csr_matrix(Xd)) for B in (Pd, sp.csr_matrix(Pd))]
    for K in Ks:
        assert isinstance(K, np.ndarray) and K.shape == (9, 7)
        np.testing.assert_allclose(K, ref, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(K, Ks[0], rtol=1e-13, atol=1e-14)
    assert np.all(Ks[0][2] == (1.0 if kind == "all-subsets" else 0.0))  # the empty row
    # dense first = transpose of the swapped call (the transpose_out path)
    np.testing.assert_allclose(f(Pd, sp.csr_matrix(Xd)), f(sp.csr_matrix(Xd), Pd).T,
                               rtol=1e-13, atol=1e-14)
    # poly_predict through the same forms
    lams = np.linspace(-1, 1, 7)
    for A in (Xd, sp.csr_matrix(Xd)):
        for B in (Pd, sp.csr_matrix(Pd)):
            np.testing.assert_allclose(km.poly_predict(A, B, lams, kind, degree), ref @ lams,
                                       rtol=1e-12, atol=1e-12)


def test_non_canonical_csr_input():
    km = _km()
    Xd, Pd = _awkward_pair(5)
    rng = np.random.RandomState(0)
    data, indices, indptr = [], [], [0]
    for i in range(Xd.shape[0]):
        ent = [(c, Xd[i, c]) for c in np.flatnonzero(Xd[i])]
        if len(ent) >= 2:  # one entry split into two duplicates that sum to it
            c, v = ent.pop(0)
            ent += [(c, 0.75 * v), (c, 0.25 * v)]
        ent = [ent[t] for t in rng.permutation(len(ent))]  # unsorted
        indices += [c for c, _ in ent]
        data += [v for _, v in ent]
        indptr.append(len(indices))
    Xn = sp.csr_matrix((np.array(data), np.array(indices, np.int32), np.array(indptr)),
                       shape=Xd.shape)
    assert not Xn.has_canonical_format
    np.testing.assert_allclose(Xn.toarray(), Xd, rtol=1e-15, atol=0)
    before = (Xn.data.copy(), Xn.indices.copy())
    for m in (2, 3):
        ref = _dp(Xn.toarray(), Pd, "anova", m)
        np.testing.assert_allclose(km.anova_kernel(Xn, Pd, m), ref, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(km.anova_kernel(Xn, sp.csr_matrix(Pd), m), ref,
                                   rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(km.anova_kernel(Pd, Xn, m), ref.T, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(Xn.data, before[0])  # the caller's matrix is left alone
    np.testing.assert_array_equal(Xn.indices, before[1])


def test_sparse_p_gives_true_anova():
    """The documented deviation: a scipy-sparse P at degree >= 2 gives the ANOVA kernel (the
    reference's _D takes a matrix power of P.T there)."""
    km = _km()
    Xd, Pd = _awkward_pair(7)
    for m in (2, 3, 4):
        np.testing.assert_allclose(km.anova_kernel(Xd, sp.csr_matrix(Pd), m),
                                   km.anova_kernel(Xd, Pd, m), rtol=1e-13, atol=1e-14)
        np.testing.assert_allclose(km.anova_kernel(sp.csc_matrix(Xd), sp.csc_matrix(Pd), m),
                                   _brute_anova(Xd, Pd, m), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ 3. brute force
def test_brute_force_tiny_d():
    km = _km()
    rng = np.random.RandomState(11)
    Xd = rng.randn(6, 8) * (rng.rand(6, 8) < 0.8)
    Pd = rng.randn(5, 8) * (rng.rand(5, 8) < 0.8)
    support = ((Xd != 0)[:, None, :] & (Pd != 0)[None, :, :]).sum(axis=2)
    for m in range(1, 11):
        ref = _brute_anova(Xd, Pd, m) if m <= 8 else np.zeros((6, 5))
        for X in (Xd, sp.csr_matrix(Xd)):
            K = km.anova_kernel(X, Pd, m)
            np.testing.assert_allclose(K, ref, rtol=1e-12, atol=1e-12)
            assert np.all(K[support < m] == 0.0)
    xpt = Xd @ Pd.T
    for m in (0, -1):
        np.testing.assert_allclose(km.anova_kernel(Xd, Pd, m), xpt, rtol=1e-13, atol=1e-14)
    with pytest.raises(NotImplementedError):
        km.anova_kernel(Xd, Pd, 65)
    K64 = km.anova_kernel(np.ones((2, 70)), np.ones((3, 70)), 64)  # C(70, 64) = 131115985
    np.testing.assert_allclose(K64, np.full((2, 3), 131115985.0), rtol=1e-12)
    for m in range(0, 6):
        for X in (Xd, sp.csr_matrix(Xd)):
            np.testing.assert_allclose(km.homogeneous_kernel(X, Pd, m), xpt ** m,
                                       rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ 4. dtypes
def test_result_dtype_follows_reference():
    km = _km()
    rng = np.random.RandomState(1)
    X32 = (rng.randn(5, 6) * (rng.rand(5, 6) < 0.7)).astype(np.float32)
    P32 = rng.randn(3, 6).astype(np.float32)
    for X in (X32, sp.csr_matrix(X32)):
        for m in (0, 1, 2, 3):
            K = km.anova_kernel(X, P32, m)
            assert K.dtype == np.float32
            np.testing.assert_allclose(K, _dp(X32.astype(np.float64), P32.astype(np.float64),
                                                "anova", m).astype(np.float32), rtol=1e-6,
                                       atol=1e-6)
        assert km.anova_kernel(X, P32, 4).dtype == np.float64
        assert km.homogeneous_kernel(X, P32, 3).dtype == np.float32
        assert km.all_subsets_kernel(X, P32).dtype == np.float64
        assert km.anova_kernel(X, P32.astype(np.float64), 2).dtype == np.float64
        assert km.poly_predict(X, P32, np.ones(3, np.float32), "anova", 2).dtype == np.float32
        assert km.poly_predict(X, P32, np.ones(3), "anova", 2).dtype == np.float64
    assert km.homogeneous_kernel(X32.astype(np.float64), P32, 2).dtype == np.float64


# ------------------------------------------------------------------ 5. lane / LDS boundaries
@pytest.mark.parametrize("n2", [1, 31, 32, 33, 63, 64, 65, 129])
def test_lane_boundaries(n2):
    km = _km()
    rng = np.random.RandomState(n2)
    Xs = _sparse_x(70, 40, 0.15, n2).tolil()
    Xs[0, :] = 0
    Xs[1, :] = 0
    Xs[1, 7] = 1.5  # one entry
    Xs = Xs.tocsr()
    Xd = Xs.toarray()
    Pd = rng.randn(n2, 40) * (rng.rand(n2, 40) < 0.5)
    lams = rng.randn(n2)
    for kind, m in (("anova", 2), ("anova", 3), ("poly", 2), ("all-subsets", 0)):
        ref = _dp(Xd, Pd, kind, m)
        for B in (Pd, sp.csr_matrix(Pd)):
            K = km._gram(Xs, B, kind, m)
            np.testing.assert_allclose(K, ref, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(km._gram(Xs, B, kind, m, lams=lams), ref @ lams,
                                       rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(km._gram(Pd, Xs, kind, m), ref.T, rtol=1e-12, atol=1e-12)


def test_long_rows_overflow_lds_staging():
    """A row of X longer than the dense path's staging round (1024 entries) and a 64-row chunk of
    P whose entries overflow the CSR path's staging space (2048): the global-memory path."""
    km = _km()
    rng = np.random.RandomState(4)
    d = 3000
    Xd = rng.randn(40, d) * (rng.rand(40, d) < 0.01)
    Xd[3] = rng.randn(d) * (rng.rand(d) < 0.8)  # ~2400 entries
    Xd[4] = 0.0
    Pd = rng.randn(70, d) * (rng.rand(70, d) < 0.02)
    Pd[10] = rng.randn(d) * (rng.rand(d) < 0.9)  # its chunk holds > 2048 entries
    Pd[11] = 0.0
    lams = rng.randn(70)
    for kind, m in (("anova", 2), ("anova", 4), ("poly", 2), ("all-subsets", 0)):
        ref = _dp(Xd, Pd, kind, m)
        tol = 1e-10 * max(1.0, float(np.abs(ref).max()))
        for B in (Pd, sp.csr_matrix(Pd)):
            np.testing.assert_allclose(km._gram(sp.csr_matrix(Xd), B, kind, m), ref, rtol=1e-10,
                                       atol=tol)
            np.testing.assert_allclose(km._gram(sp.csr_matrix(Xd), B, kind, m, lams=lams),
                                       ref @ lams, rtol=1e-10, atol=tol * 10)


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("p_sparse", [False, True])
def test_block_budget_and_repeats_are_bit_identical(p_sparse):
    km = _km()
    rng = np.random.RandomState(8)
    Xs = _sparse_x(3000, 50, 0.2, 8)
    Pd = rng.randn(200, 50) * (rng.rand(200, 50) < 0.5)
    B = sp.csr_matrix(Pd) if p_sparse else Pd
    lams = rng.randn(200)
    for kind, m in (("anova", 3), ("poly", 2), ("all-subsets", 0)):
        K0 = km._gram(Xs, B, kind, m)
        K1 = km._gram(Xs, B, kind, m)
        Kt = km._gram(Xs, B, kind, m, max_block_bytes=48 << 10)  # 64-column tiles, row blocks
        assert np.array_equal(K0, K1) and np.array_equal(K0, Kt)
        y0 = km._gram(Xs, B, kind, m, lams=lams)
        y1 = km._gram(Xs, B, kind, m, lams=lams)
        yt = km._gram(Xs, B, kind, m, lams=lams, max_block_bytes=48 << 10)
        assert np.array_equal(y0, y1) and np.array_equal(y0, yt)
        np.testing.assert_allclose(y0, K0 @ lams, rtol=1e-11, atol=1e-11)
    KT0 = km._gram(Pd, Xs, "anova", 2)
    KTt = km._gram(Pd, Xs, "anova", 2, max_block_bytes=48 << 10)
    assert np.array_equal(KT0, KTt)


# ------------------------------------------------------------------ 7. medium sizes vs oracle
def test_medium_random_against_oracle():
    from oracle import oracle as orc

    km = _km()
    rng = np.random.RandomState(12)
    Xs = _sparse_x(20000, 5000, 0.004, 12)
    P = rng.randn(30, 5000)
    for m in (2, 3, 4):
        ref = orc.anova_kernel(Xs, P, m)
        K = km.anova_kernel(Xs, P, m)
        # the reference's closed forms cancel large terms: relative to the size of those terms
        scale = np.abs(Xs).dot(np.abs(P).T) ** m
        assert np.all(np.abs(K - ref) <= 1e-11 * scale + 1e-12)
        Kh = km.homogeneous_kernel(Xs, P, m)
        np.testing.assert_allclose(Kh, orc.homogeneous_kernel(Xs, P, m), rtol=1e-10,
                                   atol=1e-12 * float(np.abs(scale).max()))


# ------------------------------------------------------------------ 8. large, vs HipEngine.predict
def test_large_poly_predict_against_engine_predict():
    from sparsepoly_amd.engine import HipEngine
    from sparsepoly_amd.synth import make_csr

    km = _km()
    X = make_csr(250_000, 100_000, nnz_per_row=50, seed=5)
    rng = np.random.RandomState(5)
    P = rng.randn(30, 100_000) * 0.1
    lams = np.sign(rng.randn(30))
    y = km.poly_predict(X, P, lams, "anova", 2)
    eng = HipEngine(0, "f64")
    try:
        eng.set_params(P[None], np.zeros(100_000), lams)
        ref = eng.predict(X, 2, False, False)
    finally:
        eng.close()
    np.testing.assert_allclose(y, ref, rtol=1e-10, atol=1e-10 * float(np.abs(ref).max()))
    # several row blocks
    yb = km._gram(X, P, "anova", 2, lams=lams, max_block_bytes=64 << 20)
    assert np.array_equal(y, yb)
