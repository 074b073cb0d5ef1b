"""Why a row got its prediction: per-row feature attributions of a fitted factorization machine,
on the device.

Every term of the model is a monomial in the row's entries.  Against the baseline ``x = 0`` the
Shapley value of a monomial splits it equally among its members, so the attribution of the stored
entry ``(i, j)`` is exact and cheap,

    phi_ij = w_j x_ij + x_ij sum_blocks sum_s lams_s p_sj sum_t (c_st / t) A^{t-1}(p_s, x_i without j)

and ``sum_j phi_ij + base = decision_function(X)_i``.  ``A^{t-1}(.. without j)`` is the downdate
``g_0 = 1, g_t = a_t - p_sj x_ij g_{t-1}`` of the row's own kernels ``a_t``.  The same pass with
``c_st`` in place of ``c_st / t`` and without the leading ``x_ij`` is the input gradient
(``spfm_explain_*``, ``include/spfm.h``).  There is no CPU path: without the
library or a GPU the device calls raise.

A block of the model is ``sum_s lams_s sum_t c[s][t] A^t(p_s, x)`` with a coefficient table
``c`` (k, 7).  A plain block of degree M has ``c[s][M] = 1``.  With ``fit_lower='augment'`` the
dummy columns never reach the device: ``A^M`` over the real and the dummy columns splits into
``sum_t A^{M-t}(dummies) A^t(real)``, so ``c[s][t] = A^{M-t}(p_s over the dummy columns, 1)`` and
the engine sees ``P_``, ``w_`` restricted to the real columns and the caller's own ``X``.

``ExplainMixin`` gives the factorization-machine estimators ``feature_contributions``,
``input_gradient`` and ``top_contributions``.  The all-subsets estimators do not have it: the
Shapley split of their product needs every order up to the row length.
``restate_contributions`` is the plain NumPy restatement, a test aid that never touches the device.
"""
import numpy as np
import scipy.sparse as sp

from . import _capi
from .ranking import _canonical, _spec

MODES = tuple(_capi.EXPLAIN_MODES)


def _columns(est, d):
    """(real, dummy): where ``_augment`` puts the d real columns and its dummy columns, found by
    probing it with an empty row"""
    probe = sp.csr_matrix(est._augment(sp.csr_matrix((1, d), dtype=np.double)))
    dummy = np.sort(probe.indices)
    return np.setdiff1d(np.arange(probe.shape[1]), dummy), dummy


def _model(est, X, dtype=np.double):
    """Checked canonical ``X`` and the model form the engine is handed: ``(Xc, blocks, coef, P, w,
    lams, lin, base)`` -- ``blocks`` the (order index, degree) pairs of ``_get_output``, ``coef``
    (n_blocks, k, 7), ``P`` (n_orders, k, d) and ``w`` (d) over the real columns.  Every argument
    error is raised here, before a handle exists."""
    degree, lin, lower, P, w, lams = _spec(est)
    Xc = _canonical(X)
    d = Xc.shape[1]
    real, dummy = _columns(est, d)
    if real.size + dummy.size != P.shape[2]:
        raise ValueError("X has %d features, the model was fitted on %d"
                         % (d, P.shape[2] - dummy.size))
    blocks = [(0, degree)] + ([(1, 2)] if lower else [])
    k = P.shape[1]
    coef = np.zeros((len(blocks), k, 7), dtype=dtype)
    for q, (o, m) in enumerate(blocks):
        # a[u] = A^u(p_s over the dummy columns, values 1), by the recurrence over the columns
        a = [np.ones(k, dtype=dtype)] + [np.zeros(k, dtype=dtype) for _ in range(m)]
        for j in dummy:
            for u in range(m, 0, -1):
                a[u] = a[u] + a[u - 1] * P[o, :, j].astype(dtype)
        for t in range(m + 1):
            coef[q, :, t] = a[m - t]
    base = (coef[:, :, 0] * lams.astype(dtype)).sum()
    if lin:
        base = base + w[dummy].astype(dtype).sum()
    return (Xc, blocks, coef, np.ascontiguousarray(P[:, :, real]), np.ascontiguousarray(w[real]),
            lams, lin, base)


def _check_K(K):
    if int(K) != K or K < 1:
        raise ValueError("K must be an integer >= 1, got %r" % (K,))
    if K > _capi.EXPLAIN_MAX_K:
        raise ValueError("K = %d exceeds the cap of %d (SPFM_EXPLAIN_MAX_K); a larger K is "
                         "refused, never answered approximately" % (K, _capi.EXPLAIN_MAX_K))
    return int(K)


class ExplainMixin(object):
    """Shared by the factorization-machine estimators."""

    def _explain(self, X, call):
        """``call(engine, Xc, blocks, coef, lin)`` on a handle made as ``_get_output`` makes one"""
        Xc, blocks, coef, P, w, lams, lin, base = _model(self, X)
        engine = self._new_engine()
        try:
            engine.set_params(P, w, lams)
            return Xc, base, call(engine, Xc, blocks, coef, lin)
        finally:
            engine.close()

    def _explain_values(self, X, mode):
        Xc, base, (vals, _) = self._explain(
            X, lambda e, Xc, blocks, coef, lin: e.explain(Xc, blocks, coef, lin, mode,
                                                          rowsum=False))
        return sp.csr_matrix((vals, Xc.indices, Xc.indptr), shape=Xc.shape), float(base)

    def feature_contributions(self, X, return_base=False):
        """The attribution of every stored entry: a float64 ``csr_matrix`` (n, n_features) on the
        pattern of the canonical ``X`` (indices sorted, duplicates summed; the caller's arrays
        are not changed), holding the exact Shapley values of the model output against the
        baseline ``x = 0``.  Classifiers are explained in ``decision_function`` space.  Each row
        sums to ``decision_function(X)_i - base``; ``return_base``: ``(contributions, base)``,
        ``base`` the model's output on an empty row."""
        out, base = self._explain_values(X, "attribution")
        return (out, base) if return_base else out

    def input_gradient(self, X):
        """``d f / d x_ij`` on the stored entries of the canonical ``X``, as a float64
        ``csr_matrix`` of the same pattern.  It is the derivative with respect to a stored entry
        with the sparsity pattern held fixed: a column that a row does not store has a
        derivative too (in general not zero), and it is not reported."""
        return self._explain_values(X, "gradient")[0]

    def top_contributions(self, X, K):
        """``(cols, vals)``, int32 and float64 of shape (n, K): per row its ``min(K, n_i)``
        attributions largest by magnitude, ordered by ``|phi|`` descending, then column
        ascending; shorter rows are padded with column -1 and value 0.  Exact and
        deterministic.  ``1 <= K <= 64``.  Only the (n, K) lists leave the device."""
        K = _check_K(K)
        return self._explain(
            X, lambda e, Xc, blocks, coef, lin: e.explain_topk(Xc, blocks, coef, lin, K))[2]


# ------------------------------------------------------------------ NumPy restatement (test aid)
def restate_contributions(est, X, mode, wide=False):
    """Test aid, NumPy only, never touches the device: the formula of the module docstring applied
    to dense rows.  ``mode``: 'attribution' or 'gradient'.  Returns ``(Xc, values, base)``: the
    canonical ``X``, one value per stored entry in the order of ``Xc.data`` and the base value,
    in ``np.longdouble`` (as is all the arithmetic) when ``wide`` is set.  Dense intermediates:
    small shapes only."""
    if mode not in MODES:
        raise ValueError("mode must be 'attribution' or 'gradient', got %r" % (mode,))
    dtype = np.longdouble if wide else np.double
    Xc, blocks, coef, P, w, lams, lin, base = _model(est, X, dtype)
    P, w, lams = P.astype(dtype), w.astype(dtype), lams.astype(dtype)
    V = np.asarray(Xc.todense(), dtype=dtype)
    n, d = V.shape
    out = np.zeros((n, d), dtype=dtype)
    used = np.flatnonzero((V != 0).any(axis=0))
    for q, (o, m) in enumerate(blocks):
        for s0 in range(0, P.shape[1], 16):  # 16 components at a time: (n, 16, d) intermediates
            Ps, c = P[o, s0:s0 + 16], coef[q, s0:s0 + 16]
            PX = Ps[None, :, :] * V[:, None, :]
            a = [np.ones(PX.shape[:2], dtype=dtype)] + [np.zeros(PX.shape[:2], dtype=dtype)
                                                        for _ in range(m)]
            for j in used:
                for t in range(m, 0, -1):
                    a[t] = a[t] + a[t - 1] * PX[:, :, j]
            g = np.ones(PX.shape, dtype=dtype)
            inner = np.zeros(PX.shape, dtype=dtype)
            for t in range(1, m + 1):
                if t > 1:
                    g = a[t - 1][:, :, None] - PX * g
                ct = c[:, t] / t if mode == "attribution" else c[:, t]
                inner = inner + ct[None, :, None] * g
            out += ((lams[s0:s0 + 16, None] * Ps)[None] * inner).sum(axis=1)
    if lin:
        out += w[None, :]
    if mode == "attribution":
        out *= V
    rows = np.repeat(np.arange(n), np.diff(Xc.indptr))
    return Xc, out[rows, Xc.indices], base
