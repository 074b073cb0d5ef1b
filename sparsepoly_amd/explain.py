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

Which *pairs* of a row's entries produced its score is the same split taken one order up, the
Shapley-Taylor interaction index of order 2: a monomial of one entry stays with that entry (its
main effect), a monomial of ``t >= 2`` entries is split equally among its ``t (t - 1) / 2`` pairs.
With ``z_sj = p_sj x_ij``, the stored entries ``a < b`` of row ``i`` get

    main_ia = w_a x_ia + sum_blocks sum_s lams_s c[s][1] z_sa
    phi_iab = sum_blocks sum_s lams_s z_sa z_sb sum_{t=2..M} c[s][t] 2 / (t (t - 1)) h_{t-2}
    g_0 = h_0 = 1,  g_t = a_t - z_sa g_{t-1},  h_t = g_t - z_sb h_{t-1}

(the downdate applied twice), ``sum_a main_ia + sum_{a<b} phi_iab + base = decision_function(X)_i``
and ``phi_ia = main_ia + 1/2 sum_{b != a} phi_iab``.  Without the ``2 / (t (t - 1))`` and the
leading ``x_ia x_ib`` it is the mixed second derivative on the stored pairs
(``spfm_explain_pairs_*``).

``ExplainMixin`` gives the factorization-machine estimators ``feature_contributions``,
``input_gradient`` and ``top_contributions``, ``pair_contributions``, ``top_pair_contributions``
and ``group_contributions``.  The all-subsets estimators do not have it: the
Shapley split of their product needs every order up to the row length.
``restate_contributions`` and ``restate_pair_contributions`` are the plain NumPy restatements,
test aids that never touch the device.
"""
import numpy as np
import scipy.sparse as sp

from . import _capi
from .ranking import _canonical, _spec

MODES = tuple(_capi.EXPLAIN_MODES)
PAIR_MODES = tuple(_capi.PAIRS_MODES)


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


def _check_K(K, cap=_capi.EXPLAIN_MAX_K, name="SPFM_EXPLAIN_MAX_K"):
    if int(K) != K or K < 1:
        raise ValueError("K must be an integer >= 1, got %r" % (K,))
    if K > cap:
        raise ValueError("K = %d exceeds the cap of %d (%s); a larger K is "
                         "refused, never answered approximately" % (K, cap, name))
    return int(K)


def _check_pair_mode(mode):
    if mode not in PAIR_MODES:
        raise ValueError("mode must be 'interaction' or 'hessian', got %r" % (mode,))


def _check_groups(groups, d):
    """-> (int32 ids, G): one id >= 0 per feature, G = the largest id + 1 within the cap"""
    g = np.asarray(groups)
    if g.shape != (d,):
        raise ValueError("groups must hold one id per feature (%d), got shape %r" % (d, g.shape))
    if not np.issubdtype(g.dtype, np.integer):
        raise ValueError("groups must be an integer array, got dtype %s" % g.dtype)
    if d and g.min() < 0:
        raise ValueError("groups must hold ids >= 0, got %d" % g.min())
    G = int(g.max()) + 1 if d else 1
    if G > _capi.PAIRS_MAX_GROUPS:
        raise ValueError("groups name %d groups, more than the cap of %d (SPFM_PAIRS_MAX_GROUPS)"
                         % (G, _capi.PAIRS_MAX_GROUPS))
    return g.astype(np.int32), G


def pair_columns(Xc):
    """``(pair_ptr, col_a, col_b)`` of a canonical CSR matrix: row ``i`` owns
    ``n_i (n_i - 1) / 2`` pairs ordered by (first position, second position); ``col_a < col_b``
    are the two members' columns."""
    n_i = np.diff(Xc.indptr).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(n_i * (n_i - 1) // 2)]).astype(np.int64)
    ca = np.zeros(int(ptr[-1]), dtype=np.int32)
    cb = np.zeros(int(ptr[-1]), dtype=np.int32)
    tri = {}
    for i in np.flatnonzero(n_i > 1):
        m = int(n_i[i])
        if m not in tri:
            tri[m] = np.triu_indices(m, 1)
        cols = Xc.indices[Xc.indptr[i]:Xc.indptr[i + 1]]
        ca[ptr[i]:ptr[i + 1]] = cols[tri[m][0]]
        cb[ptr[i]:ptr[i + 1]] = cols[tri[m][1]]
    return ptr, ca, cb


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


    def pair_contributions(self, X, mode="interaction", return_main=False, return_base=False):
        """The attribution of every pair of stored entries of a row: ``(pair_ptr, col_a, col_b,
        vals)``, flat arrays on the canonical ``X`` (indices sorted, duplicates summed): row ``i``
        owns ``vals[pair_ptr[i]:pair_ptr[i + 1]]``, its ``n_i (n_i - 1) / 2`` pairs ordered by
        (first, second) member, ``col_a < col_b`` their columns.  ``mode='interaction'``: the
        exact Shapley-Taylor interaction index of order 2 of the model output against the baseline
        ``x = 0`` (classifiers: in ``decision_function`` space); with ``return_main`` a float64
        ``csr_matrix`` ``main`` on the pattern of the canonical ``X`` follows, the part of the
        output that belongs to one entry alone, and with ``return_base`` the model's output on an
        empty row: per row ``main.sum() + vals.sum() + base = decision_function(X)_i``, and
        ``feature_contributions(X)[i, a] = main[i, a] + half the values of the pairs that hold
        a``.  ``mode='hessian'``: ``d2f / dx_ia dx_ib`` with the sparsity pattern held fixed (no
        ``main``).  A call that would list more than 1 GiB of values is refused."""
        _check_pair_mode(mode)
        if return_main and mode != "interaction":
            raise ValueError("return_main belongs to mode='interaction'")
        Xc, base, (ptr, vals, mn) = self._explain(
            X, lambda e, Xc, blocks, coef, lin: e.explain_pairs(Xc, blocks, coef, lin, mode,
                                                                main=return_main))
        ptr2, ca, cb = pair_columns(Xc)
        assert (ptr == ptr2).all()
        out = (ptr, ca, cb, vals)
        if return_main:
            out += (sp.csr_matrix((mn, Xc.indices, Xc.indptr), shape=Xc.shape),)
        if return_base:
            out += (float(base),)
        return out

    def top_pair_contributions(self, X, K, mode="interaction"):
        """``(col_a, col_b, vals)``, int32, int32 and float64 of shape (n, K): per row its
        ``min(K, n_i (n_i - 1) / 2)`` pair attributions (``mode='hessian'``: second derivatives)
        largest by magnitude, ordered by ``|value|`` descending, then first column, then second
        column ascending; rows with fewer pairs are padded with -1, -1 and 0.  Exact and
        deterministic.  ``1 <= K <= 64``.  Only the (n, K) lists leave the device."""
        K = _check_K(K, _capi.PAIRS_MAX_K, "SPFM_PAIRS_MAX_K")
        _check_pair_mode(mode)
        return self._explain(
            X, lambda e, Xc, blocks, coef, lin: e.explain_pairs_topk(Xc, blocks, coef, lin, K,
                                                                     mode))[2]

    def group_contributions(self, X, groups, return_base=False):
        """Field-level tables: ``groups`` is an int array of length ``n_features`` with ids
        ``>= 0`` (at most 32 groups, ``G`` = the largest id + 1).  Returns ``(T, main)``: ``T``
        (n, G, G) upper-triangular, ``T[i, g, h]``, ``g <= h``, the sum of row ``i``'s pair
        attributions over the pairs with one member in group ``g`` and the other in ``h`` (the
        diagonal: both in ``g``), and ``main`` (n, G) the main effects summed per group, so that
        ``T.sum((1, 2)) + main.sum(1) + base = decision_function(X)``; ``return_base``:
        ``(T, main, base)``."""
        Xc, _, _, _, _, _, _, base = _model(self, X)  # (argument errors before a handle exists)
        g, G = _check_groups(groups, Xc.shape[1])
        cells, mn = self._explain(
            X, lambda e, Xc, blocks, coef, lin: e.explain_pairs_grouped(Xc, blocks, coef, lin, G,
                                                                        g))[2]
        T = np.zeros((Xc.shape[0], G, G))
        iu = np.triu_indices(G)
        T[:, iu[0], iu[1]] = cells
        return (T, mn, float(base)) if return_base else (T, mn)


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


def restate_pair_contributions(est, X, mode, wide=False):
    """Test aid, NumPy only, never touches the device: the pair formula of the module docstring,
    row by row.  ``mode``: 'interaction' or 'hessian'.  Returns ``(Xc, pair_ptr, col_a, col_b,
    vals, main, base)``: the canonical ``X``, the pairs in the order of ``pair_contributions``,
    one ``main`` per stored entry in the order of ``Xc.data`` (zeros for 'hessian') and the base
    value, in ``np.longdouble`` (as is all the arithmetic) when ``wide`` is set.  (k, pairs)
    intermediates: small shapes only."""
    _check_pair_mode(mode)
    dtype = np.longdouble if wide else np.double
    Xc, blocks, coef, P, w, lams, lin, base = _model(est, X, dtype)
    P, w, lams = P.astype(dtype), w.astype(dtype), lams.astype(dtype)
    ptr, ca, cb = pair_columns(Xc)
    vals = np.zeros(int(ptr[-1]), dtype=dtype)
    main = np.zeros(Xc.nnz, dtype=dtype)
    for i in range(Xc.shape[0]):
        lo, hi = Xc.indptr[i], Xc.indptr[i + 1]
        cols, x = Xc.indices[lo:hi], Xc.data[lo:hi].astype(dtype)
        m = hi - lo
        if m == 0:
            continue
        ia, ib = np.triu_indices(m, 1)
        if mode == "interaction" and lin:
            main[lo:hi] += w[cols] * x
        for q, (o, M) in enumerate(blocks):
            for s0 in range(0, P.shape[1], 16):  # 16 components at a time: (16, pairs) arrays
                Pc, c, lm = P[o][s0:s0 + 16][:, cols], coef[q][s0:s0 + 16], lams[s0:s0 + 16]
                Z = Pc * x[None, :]
                a = [np.ones(Z.shape[0], dtype=dtype)] + [np.zeros(Z.shape[0], dtype=dtype)
                                                          for _ in range(M)]
                for j in range(m):
                    for t in range(M, 0, -1):
                        a[t] = a[t] + a[t - 1] * Z[:, j]
                if mode == "interaction":
                    main[lo:hi] += ((lm * c[:, 1])[:, None] * Z).sum(axis=0)
                if m < 2:
                    continue
                za, zb = Z[:, ia], Z[:, ib]
                g = np.ones(za.shape, dtype=dtype)
                h = np.ones(za.shape, dtype=dtype)
                inner = np.zeros(za.shape, dtype=dtype)
                for t in range(2, M + 1):
                    if t > 2:
                        g = a[t - 2][:, None] - za * g
                        h = g - zb * h
                    ct = c[:, t] * 2 / (t * (t - 1)) if mode == "interaction" else c[:, t]
                    inner = inner + ct[:, None] * h
                lead = za * zb if mode == "interaction" else Pc[:, ia] * Pc[:, ib]
                vals[ptr[i]:ptr[i + 1]] += (lm[:, None] * lead * inner).sum(axis=0)
    return Xc, ptr, ca, cb, vals, main, base
