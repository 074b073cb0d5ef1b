"""Kernel (Gram) matrices and ``poly_predict`` -- counterpart of the reference's
``sparsepoly/kernels.py`` (:14-153), with the same names, signatures and argument order.

==========================================  ==================================================
``safe_power(X, degree=2)``                 element-wise power, sparse or dense (host only)
``homogeneous_kernel(X, P, degree=2)``      ``(X P^T) ** degree``
``anova_kernel(X, P, degree=2)``            ANOVA kernel of order ``degree``
``all_subsets_kernel(X, P)``                ``prod_c (1 + x_c p_c)``
``poly_predict(X, P, lams, kernel, deg)``   ``K(X, P) @ lams``
==========================================  ==================================================

The four kernel functions run on the GPU (``spfm_gram_csr_dense`` / ``spfm_gram_csr_csr`` of
``include/spfm.h``) and take one keyword-only ``device=None`` (default: the estimators' device,
``LOCAL_RANK`` or 0).  There is no CPU fallback: without the built library or a GPU they raise
``SpfmError``.  ``X`` and ``P`` may each be dense or scipy-sparse; both must be 2-D with the same
number of features (``ValueError`` otherwise, before any device work).  The result is always a
host ``numpy.ndarray`` (never a sparse matrix).  Values are computed in float64 on the device
and rounded once at the end to the reference's result type: float32 for ``homogeneous_kernel``
and for ``anova_kernel`` with degree <= 3 when both inputs are float32, float64 otherwise.
``poly_predict`` reduces ``K @ lams`` on the device in the pass that evaluates ``K``; the
``n1 x n2`` matrix is never formed.

Degrees follow the reference: ``anova_kernel`` with degree <= 1 returns ``X P^T`` (its
else-branch with an empty recursion, also for 0 and negative degrees); a degree above a pair's
number of common nonzeros gives exactly 0; degrees above ``SPFM_GRAM_MAX_DEGREE`` (64) raise
``NotImplementedError``.  ``homogeneous_kernel`` takes integer degrees >= 0 (else
``NotImplementedError``).

One deliberate deviation: with a scipy-sparse ``P``, the reference's ``anova_kernel`` at degree
>= 2 evaluates ``P.T ** degree`` as a *matrix* power (``_D``, kernels.py:43-48), which raises
``TypeError`` for a non-square ``P`` and silently returns a wrong value for a square one.  This
module returns the true ANOVA kernel for sparse ``P`` as well.
"""
import numbers

import numpy as np
import scipy.sparse as sp

from . import _capi
from .engine import HipEngine, SpfmError

__all__ = ["safe_power", "homogeneous_kernel", "anova_kernel", "all_subsets_kernel",
           "poly_predict"]


def safe_power(X, degree=2):
    """Element-wise power supporting both sparse and dense data (kernels.py:14-40)."""
    if sp.issparse(X):
        if hasattr(X, "power"):
            return X.power(degree)
        X = X.copy()
        X.data **= degree
        return X
    return X ** degree


# ------------------------------------------------------------------ host-side checks
def _operand(A, name):
    if sp.issparse(A):
        if len(A.shape) != 2:
            raise ValueError("%s must be 2-D, got shape %r" % (name, A.shape))
        return A
    A = np.asarray(A)
    if A.ndim != 2:
        raise ValueError("%s must be 2-D, got shape %r" % (name, A.shape))
    return A


def _pair(X, P):
    X, P = _operand(X, "X"), _operand(P, "P")
    if X.shape[1] != P.shape[1]:
        raise ValueError("X has %d features, P has %d" % (X.shape[1], P.shape[1]))
    return X, P


def _int_degree(degree):
    if isinstance(degree, (bool, np.bool_)):
        return None
    if isinstance(degree, numbers.Integral):
        return int(degree)
    if isinstance(degree, numbers.Real) and float(degree).is_integer():
        return int(degree)
    return None


def _anova_degree(degree):
    m = _int_degree(degree)
    if m is None:
        raise NotImplementedError("anova_kernel: integer degree required, got %r" % (degree,))
    if m > _capi.GRAM_MAX_DEGREE:
        raise NotImplementedError("anova_kernel: degree %d above SPFM_GRAM_MAX_DEGREE (%d)"
                                  % (m, _capi.GRAM_MAX_DEGREE))
    return max(m, 1)


def _poly_degree(degree):
    m = _int_degree(degree)
    if m is None or m < 0:
        raise NotImplementedError("homogeneous_kernel: integer degree >= 0 required, got %r"
                                  % (degree,))
    return m


def _both_f32(X, P):
    return X.dtype == np.float32 and P.dtype == np.float32


def _result_dtype(kind, degree, X, P):
    """The reference's result type (float32 only where its closed forms stay in float32)."""
    if kind == "poly" and _both_f32(X, P):
        return np.float32
    if kind == "anova" and degree <= 3 and _both_f32(X, P):
        return np.float32
    return np.float64


def _csr(A):
    """float64 CSR with sorted, duplicate-free indices (duplicates summed, as scipy does);
    the caller's matrix is never modified."""
    if sp.issparse(A):
        R = sp.csr_matrix(A, dtype=np.float64)
        if not R.has_canonical_format:
            R = R.copy()  # R may share the caller's arrays
            R.sum_duplicates()
        return R
    return sp.csr_matrix(np.asarray(A, dtype=np.float64))


def _engine(device):
    if device is None:
        from .sparse_factorization_machines import _default_device

        device = _default_device()
    try:
        _capi.load()
    except RuntimeError as e:
        raise SpfmError(str(e))
    return HipEngine(device=int(device), precision="f64")


# ------------------------------------------------------------------ device call
def _gram(X, P, kind, degree, lams=None, device=None, max_block_bytes=0):
    """K(X, P) (lams None, shape (n1, n2)) or K(X, P) @ lams (shape (n1,)), float64.  X, P are
    checked 2-D operands; degree already normalised.  ``max_block_bytes``: device memory of one
    block of the work (0 = the library's default)."""
    n1, n2, d = X.shape[0], P.shape[0], X.shape[1]
    code = _capi.GRAM_KINDS[kind]
    if lams is not None:
        lams = np.ascontiguousarray(lams, dtype=np.float64)
        if lams.ndim != 1 or lams.shape[0] != n2:
            raise ValueError("lams must have shape (%d,), got %r" % (n2, lams.shape))
    x_dense, p_dense = not sp.issparse(X), not sp.issparse(P)
    transpose = lams is None and x_dense and not p_dense
    if transpose:  # K(dense, sparse) = K(sparse, dense)^T, written in place
        A, B = _csr(P), np.ascontiguousarray(X, dtype=np.float64)
    else:
        A = _csr(X)
        B = np.ascontiguousarray(P, dtype=np.float64) if p_dense else _csr(P)
    out = np.empty(n1 if lams is not None else (n1, n2), dtype=np.float64)
    ip = _capi.i64(A.indptr)
    ix = _capi.i32(A.indices)
    dv = _capi.f64(A.data)
    lp = lams.ctypes.data_as(_capi._dp) if lams is not None else None
    op = out.ctypes.data_as(_capi._dp)
    eng = _engine(device)
    try:
        if isinstance(B, np.ndarray):
            eng._check(eng._lib.spfm_gram_csr_dense(
                eng._h, code, int(degree), A.shape[0], d, ip[1], ix[1], dv[1], B.shape[0],
                B.ctypes.data_as(_capi._dp), lp, int(transpose), int(max_block_bytes), op))
        else:
            jp = _capi.i64(B.indptr)
            jx = _capi.i32(B.indices)
            jv = _capi.f64(B.data)
            eng._check(eng._lib.spfm_gram_csr_csr(
                eng._h, code, int(degree), A.shape[0], d, ip[1], ix[1], dv[1], B.shape[0],
                jp[1], jx[1], jv[1], lp, int(max_block_bytes), op))
    finally:
        eng.close()
    return out


def _cast(K, dtype):
    return K if K.dtype == dtype else K.astype(dtype)


# ------------------------------------------------------------------ public kernels
def homogeneous_kernel(X, P, degree=2, *, device=None):
    """Homogeneous polynomial kernel ``K_P(x, p) = <x, p> ** degree`` (kernels.py:51-68).
    Returns an ndarray of shape (n_samples_1, n_samples_2)."""
    X, P = _pair(X, P)
    m = _poly_degree(degree)
    return _cast(_gram(X, P, "poly", m, device=device), _result_dtype("poly", m, X, P))


def anova_kernel(X, P, degree=2, *, device=None):
    """ANOVA kernel ``K_A(x, p) = sum_{i1 > ... > id} x_i1 p_i1 ... x_id p_id``
    (kernels.py:71-115).  Returns an ndarray of shape (n_samples_1, n_samples_2)."""
    X, P = _pair(X, P)
    m = _anova_degree(degree)
    raw = _int_degree(degree)
    return _cast(_gram(X, P, "anova", m, device=device), _result_dtype("anova", raw, X, P))


def all_subsets_kernel(X, P, *, device=None):
    """All-subsets kernel ``prod_c (1 + x_c p_c)`` (kernels.py:117-137), float64."""
    X, P = _pair(X, P)
    return _gram(X, P, "all-subsets", 0, device=device)


def poly_predict(X, P, lams, kernel, degree=2, *, device=None):
    """``K(X, P) @ lams`` for kernel 'anova', 'poly' or 'all-subsets' (kernels.py:140-153),
    reduced on the device without forming K."""
    if kernel not in ("anova", "poly", "all-subsets"):
        raise ValueError(
            ("Unsuppported kernel: {}. Use one of {{'anova'|'poly'|'all-subsets'}}").format(kernel)
        )
    X, P = _pair(X, P)
    lams = np.asarray(lams)
    if kernel == "anova":
        m = _anova_degree(degree)
        kdt = _result_dtype("anova", _int_degree(degree), X, P)
    elif kernel == "poly":
        m = _poly_degree(degree)
        kdt = _result_dtype("poly", m, X, P)
    else:
        m, kdt = 0, np.float64
    out = _gram(X, P, kernel, m, lams=lams, device=device)
    return _cast(out, np.result_type(kdt, lams.dtype))
