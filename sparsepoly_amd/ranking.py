"""Rank candidates for a batch of context rows with a fitted model, on the device.

Given contexts ``X`` (B, d) -- user and context features -- and a catalogue of candidates ``Z``
(C, d) -- item id and item attributes -- over the estimator's own features, ``score[b, c]`` is
the value ``decision_function`` gives for the row ``x_b + z_c``.  The columns with a stored entry
in ``X`` and those with a stored entry in ``Z`` must be disjoint (the field structure of a
recommender).  Then the ANOVA kernel splits, ``a^m(x + z) = sum_t a^t(x) a^(m-t)(z)``, and so does
the all-subsets product, so

    score[b, c] = f(x_b) + f(z_c) + sum_blocks sum_s lams_s sum_{t=1..m-1} a_s^t(x_b) a_s^{m-t}(z_c)

is a rank-R product of two "towers" plus a constant per row and per column
(``spfm_rank_*``, ``include/spfm.h``).  Nothing of size B x C is formed
unless the dense matrix is asked for.  There is no CPU path: without the library or a GPU the
device calls raise.

``RankingMixin`` gives the estimators ``ranker``, ``candidate_scores`` and ``top_candidates``.
``restate_scores`` is the plain NumPy restatement, a test aid that never touches the device.
"""
import numpy as np
import scipy.sparse as sp
from sklearn.utils.validation import NotFittedError, check_array

from . import _capi


def _canonical(M):
    """check_array, then canonical CSR: sorted indices, duplicates summed (always a copy)"""
    M = check_array(M, accept_sparse=("csr", "csc"), dtype=np.double)
    Mr = sp.csr_matrix(M, copy=True)  # the caller's arrays are never changed
    Mr.sum_duplicates()
    Mr.sort_indices()
    return Mr


def _check_disjoint(X, Z):
    both = np.intersect1d(np.unique(X.indices), np.unique(Z.indices))
    if both.size:
        raise ValueError("column %d has stored entries in the contexts and in the candidates: the "
                         "two column sets must be disjoint (%d columns overlap)"
                         % (int(both[0]), both.size))


def _spec(est):
    """-> (degree or -1, fit_linear, add_lower_deg2, P (n_orders, k, d'), w (d'), lams)"""
    if not hasattr(est, "P_"):
        raise NotFittedError("Estimator not fitted.")
    degree, fit_linear, add_lower = est._obj_pred_args()
    P = np.ascontiguousarray(est.P_, dtype=np.double)
    P = P[None] if P.ndim == 2 else P
    w = getattr(est, "w_", None)
    w = np.zeros(P.shape[2]) if w is None else np.asarray(w, dtype=np.double)
    return degree, bool(fit_linear), bool(add_lower), P, w, np.asarray(est.lams_, dtype=np.double)


def _widen(est, X, Z):
    """The two sides over the stored block's columns.  ``fit_lower='augment'``: the dummy columns
    belong to the contexts (``X`` goes through ``_augment``), ``Z`` gets empty columns there."""
    aug = getattr(est, "_augment", None)
    if aug is None:
        return X, Z
    d = X.shape[1]
    probe = sp.csr_matrix(aug(sp.csr_matrix((1, d), dtype=np.double)))
    if probe.shape[1] == d:
        return X, Z
    dummy = probe.indices
    real = np.setdiff1d(np.arange(probe.shape[1]), dummy)  # where the d real columns went
    Xa = sp.csr_matrix(aug(X))
    Xa.sort_indices()
    Za = sp.csr_matrix((Z.data, real[Z.indices].astype(np.int32), Z.indptr),
                       shape=(Z.shape[0], probe.shape[1]))
    Za.sort_indices()
    return Xa, Za


def _prepare(est, X, Z):
    """Checked, canonical, widened (X, Z) of one width; every argument error is raised here,
    before a handle exists."""
    d_model = _spec(est)[3].shape[2]
    if X is not None:
        X = _canonical(X)
    Z = _canonical(Z)
    d = Z.shape[1]
    if X is None:  # the candidates alone: one empty context row stands in
        X = sp.csr_matrix((1, d), dtype=np.double)
    if X.shape[1] != d:
        raise ValueError("X has %d features, Z has %d" % (X.shape[1], d))
    if Z.shape[0] < 1:
        raise ValueError("Z has no rows")
    _check_disjoint(X, Z)
    Xa, Za = _widen(est, X, Z)
    if Xa.shape[1] != d_model:
        raise ValueError("X and Z have %d features, the model was fitted on %d"
                         % (d, d_model - (Xa.shape[1] - d)))
    return Xa, Za


def _check_K(K):
    if int(K) != K or K < 1:
        raise ValueError("K must be an integer >= 1, got %r" % (K,))
    if K > _capi.RANK_MAX_K:
        raise ValueError("K = %d exceeds the cap of %d (SPFM_RANK_MAX_K); a larger K is refused, "
                         "never answered approximately" % (K, _capi.RANK_MAX_K))
    return int(K)


class Ranker(object):
    """The candidates ``Z`` resident on a device handle of its own (made from ``P_``, ``w_``,
    ``lams_`` as ``predict`` makes one).  ``scores(X)`` / ``top_k(X, K)`` for any number of context
    batches; ``close()`` (or leaving the ``with`` block) releases the handle.  Not picklable."""

    def __init__(self, est, Z):
        self._est = est
        self._engine = None
        degree, lin, lower, P, w, lams = _spec(est)
        _, Za = _prepare(est, None, Z)
        self._Z = _canonical(Z)
        self.n_candidates = Za.shape[0]
        engine = est._new_engine()
        try:
            engine.set_params(P, w, lams)
            engine.rank_set_candidates(Za, degree, lin, lower)
        except Exception:
            engine.close()
            raise
        self._engine = engine

    def _contexts(self, X):
        if self._engine is None:
            raise ValueError("this Ranker is closed")
        Xa, _ = _prepare(self._est, X, self._Z)
        return Xa

    def scores(self, X):
        """float64 (B, C): ``score[b, c]`` = the model's output on ``x_b + z_c``.  Refused above
        1 GiB of result."""
        Xa = self._contexts(X)
        return self._engine.rank_scores(Xa)

    def top_k(self, X, K):
        """``(idx, scores)``: int32 and float64 of shape (B, min(K, C)); per context row the
        largest scores, ordered by (score descending, candidate index ascending).  Exact and
        deterministic.  ``1 <= K <= 128``."""
        K = _check_K(K)
        Xa = self._contexts(X)
        return self._engine.rank_topk(Xa, K)

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __reduce__(self):
        raise TypeError("a Ranker holds a device handle and cannot be pickled")


class RankingMixin(object):
    """Shared by the factorization-machine and all-subsets estimators."""

    def ranker(self, Z):
        """A ``Ranker`` with the candidate rows ``Z`` (C, n_features) resident on the device."""
        return Ranker(self, Z)

    def candidate_scores(self, X, Z):
        """One-shot ``ranker(Z).scores(X)``: float64 (B, C)."""
        _prepare(self, X, Z)  # argument errors before a handle is created
        with Ranker(self, Z) as r:
            return r.scores(X)

    def top_candidates(self, X, Z, K):
        """One-shot ``ranker(Z).top_k(X, K)``: ``(idx, scores)`` of shape (B, min(K, C))."""
        _check_K(K)
        _prepare(self, X, Z)
        with Ranker(self, Z) as r:
            return r.top_k(X, K)


# ------------------------------------------------------------------ NumPy restatement (test aid)
def _anova_all(PX, m, dtype):
    """a[t] (t = 0..m), each (n, k): the ANOVA kernels of every order of the rows of PX (n, k, d)
    by the recurrence a[t] += a[t-1] * p x over the features"""
    n, k, d = PX.shape
    a = [np.ones((n, k), dtype=dtype)] + [np.zeros((n, k), dtype=dtype) for _ in range(m)]
    for j in range(d):
        for t in range(m, 0, -1):
            a[t] = a[t] + a[t - 1] * PX[:, :, j]
    return a


def _restate_output(V, degree, lin, lower, P, w, lams, dtype):
    """The model's output on the dense rows V (n, d'): what ``_get_output`` computes"""
    V = np.asarray(V, dtype=dtype)
    P, w, lams = P.astype(dtype), w.astype(dtype), lams.astype(dtype)
    PX = P[0][None, :, :] * V[:, None, :]
    if degree == -1:
        return (np.prod(1 + PX, axis=2) * lams).sum(axis=1)
    out = (_anova_all(PX, degree, dtype)[degree] * lams).sum(axis=1)
    if lower:
        out = out + (_anova_all(P[1][None] * V[:, None, :], 2, dtype)[2] * lams).sum(axis=1)
    if lin:
        out = out + V @ w
    return out


def restate_scores(est, X, Z, wide=False):
    """Test aid, NumPy only, never touches the device: the (B, C) scores by evaluating the ANOVA
    recurrence (or the all-subsets product) on every summed row ``x_b + z_c`` -- no use of the
    decomposition.  ``wide``: in ``np.longdouble``.  Dense (B*C, d) intermediates: small shapes
    only."""
    degree, lin, lower, P, w, lams = _spec(est)
    Xa, Za = _prepare(est, X, Z)
    dtype = np.longdouble if wide else np.double
    Xd, Zd = np.asarray(Xa.todense(), dtype=dtype), np.asarray(Za.todense(), dtype=dtype)
    B, C = Xd.shape[0], Zd.shape[0]
    out = np.zeros((B, C), dtype=dtype)
    for b in range(B):
        out[b] = _restate_output(Xd[b][None, :] + Zd, degree, lin, lower, P, w, lams, dtype)
    return out
