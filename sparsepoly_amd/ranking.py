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

Two further consumers of the same score tiles: ``top_k(..., exclude=E)``
leaves out, per context row, the candidates that row already has, and ``ranks`` / ``evaluate``
give the exact rank of held-out candidates against the whole catalogue and the usual metrics of
it (``metrics_from_ranks``: plain NumPy on the ranks, no device).

``RankingMixin`` gives the estimators ``ranker``, ``candidate_scores``, ``top_candidates`` and
``rank_metrics``.
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


def _pattern(M, B, C, what):
    """The pattern of a (B, C) matrix of per-row candidate lists as canonical CSR (a copy with
    sorted indices, duplicates merged, every stored entry 1)"""
    if not sp.issparse(M):
        M = sp.csr_matrix(np.asarray(M))
    if M.shape != (B, C):
        raise ValueError("%s has shape %r, expected (%d contexts, %d candidates)"
                         % (what, tuple(M.shape), B, C))
    M = M.tocsr()
    if M.indices.size and (M.indices.min() < 0 or M.indices.max() >= C):
        raise ValueError("%s: candidate id out of range [0, %d)" % (what, C))
    out = sp.csr_matrix((np.ones(M.indices.shape[0]), M.indices.copy(), M.indptr.copy()),
                        shape=(B, C))
    out.sum_duplicates()
    out.sort_indices()
    out.data[:] = 1.0
    return out


def check_rank_lists(B, C, targets, exclude=None):
    """The input checks of ``Ranker.ranks`` / ``evaluate`` / ``top_k(exclude=...)``; needs no
    device.  ``targets`` and ``exclude`` are (B, C) matrices (scipy sparse or array-like) of which
    only the pattern is read.  Returns their canonical CSR patterns ``(T, E)`` (``None`` for a
    ``None``): indices sorted, duplicates merged.  ``ValueError`` for a wrong shape, a candidate id
    outside ``[0, C)``, a target that is also excluded and a row with more than
    ``SPFM_RANK_MAX_TARGETS`` targets (such a row is never truncated)."""
    T = None if targets is None else _pattern(targets, B, C, "targets")
    E = None if exclude is None else _pattern(exclude, B, C, "exclude")
    if T is not None:
        most = int(np.diff(T.indptr).max(initial=0))
        if most > _capi.RANK_MAX_TARGETS:
            row = int(np.argmax(np.diff(T.indptr)))
            raise ValueError("row %d has %d targets, more than the cap of %d "
                             "(SPFM_RANK_MAX_TARGETS); a row is never truncated"
                             % (row, most, _capi.RANK_MAX_TARGETS))
    if T is not None and E is not None:
        both = T.multiply(E).tocoo()
        if both.nnz:
            raise ValueError("candidate %d is a target of row %d and excluded from it "
                             "(%d such pairs): targets and exclude must be disjoint"
                             % (int(both.col[0]), int(both.row[0]), both.nnz))
    return T, E


def _check_ks(ks):
    ks = tuple(ks)
    for k in ks:
        if int(k) != k or k < 1:
            raise ValueError("ks must hold integers >= 1, got %r" % (k,))
    return tuple(int(k) for k in ks)


def metrics_from_ranks(tptr, ranks, n_eff, ks=(10,)):
    """Ranking metrics from exact ranks; NumPy only.  ``tptr`` (B + 1): the targets of row b are
    ``ranks[tptr[b]:tptr[b + 1]]``, 0-based among the row's ``n_eff[b]`` admissible candidates
    (targets included); a rank of -1 (a score that is not finite) counts as a miss.  Per row with
    ``n`` targets and per ``k`` in ``ks``:

    * ``recall@k`` = #{rank < k} / n, ``hit@k`` = 1 if any rank < k else 0;
    * ``ndcg@k`` = sum over the ranks < k of 1 / log2(rank + 2), over the same sum for ranks
      0 .. min(n, k) - 1;
    * ``mrr`` = 1 / (smallest rank + 1), 0 when every target is a miss;
    * ``auc`` = 1 - sum_i (r_(i) - i) / (n (n_eff - n)) with the ranks sorted ascending: the share
      of (target, other candidate) pairs the model orders correctly; a miss loses all its pairs;
      NaN when ``n_eff == n``.

    Returns a dict: each name -> its mean over the rows that have a target (``auc``: over those
    where it is defined; NaN when there is no such row), ``n_rows_scored`` -> their number,
    ``per_row`` -> a dict of the (B,) arrays (NaN for a row without targets) and ``n_targets``."""
    ks = _check_ks(ks)
    tptr = np.asarray(tptr, dtype=np.int64)
    ranks = np.asarray(ranks, dtype=np.int64)
    n_eff = np.asarray(n_eff, dtype=np.int64)
    B = tptr.shape[0] - 1
    if n_eff.shape != (B,) or ranks.shape != (int(tptr[-1]),):
        raise ValueError("tptr, ranks and n_eff do not fit together")
    n = np.diff(tptr)
    rows = np.repeat(np.arange(B), n)
    have = n > 0
    nf = np.where(have, n, 1).astype(np.double)
    valid = ranks >= 0

    def per_row_sum(w):
        return np.bincount(rows, weights=w, minlength=B)

    def blank(a):
        return np.where(have, a, np.nan)

    per = {"n_targets": n}
    gain = 1.0 / np.log2(np.where(valid, ranks, 0) + 2.0)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(max(ks)) + 2.0))])
    for k in ks:
        hit = valid & (ranks < k)
        per["recall@%d" % k] = blank(per_row_sum(hit) / nf)
        per["hit@%d" % k] = blank((per_row_sum(hit) > 0).astype(np.double))
        per["ndcg@%d" % k] = blank(per_row_sum(np.where(hit, gain, 0.0))
                                   / ideal[np.maximum(np.minimum(n, k), 1)])
    best = np.full(B, np.iinfo(np.int64).max)
    np.minimum.at(best, rows[valid], ranks[valid])
    found = best < np.iinfo(np.int64).max
    per["mrr"] = blank(np.where(found, 1.0 / (np.where(found, best, 0) + 1.0), 0.0))
    # sum_i (r_(i) - i): the ranks count the row's other targets too; a miss is beaten by all
    nv = per_row_sum(valid)
    lost = per_row_sum(np.where(valid, ranks, 0)) - nv * (nv - 1) / 2 + (n - nv) * (n_eff - n)
    pairs = (n * (n_eff - n)).astype(np.double)
    per["auc"] = np.where(pairs > 0, 1.0 - lost / np.where(pairs > 0, pairs, 1.0), np.nan)
    out = {"n_rows_scored": int(have.sum()), "per_row": per}
    for name, a in per.items():
        if name != "n_targets":
            ok = have & ~np.isnan(a)
            out[name] = float(a[ok].mean()) if ok.any() else float("nan")
    return out


class Ranker(object):
    """The candidates ``Z`` resident on a device handle of its own (made from ``P_``, ``w_``,
    ``lams_`` as ``predict`` makes one).  ``scores(X)`` / ``top_k(X, K)`` / ``ranks(X, targets)`` /
    ``evaluate(X, targets)`` for any number of context batches; ``close()`` (or leaving the
    ``with`` block) releases the handle.  Not picklable."""

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

    def top_k(self, X, K, exclude=None):
        """``(idx, scores)``: int32 and float64 of shape (B, min(K, C)); per context row the
        largest scores, ordered by (score descending, candidate index ascending).  Exact and
        deterministic.  ``1 <= K <= 128``.  ``exclude``: a (B, C) matrix of which only the pattern
        is read (a train-interaction matrix fits): the candidates stored in row b are left out for
        context b; a row with fewer than K candidates left ends in index -1 / NaN."""
        K = _check_K(K)
        Xa = self._contexts(X)
        if exclude is None:
            return self._engine.rank_topk(Xa, K)
        _, E = check_rank_lists(Xa.shape[0], self.n_candidates, None, exclude)
        return self._engine.rank_topk(Xa, K, exclude=(E.indptr, E.indices))

    def _rank_eval(self, X, targets, exclude):
        Xa = self._contexts(X)
        T, E = check_rank_lists(Xa.shape[0], self.n_candidates, targets, exclude)
        ranks, scores, n_eff = self._engine.rank_eval(
            Xa, (T.indptr, T.indices), None if E is None else (E.indptr, E.indices))
        return T, ranks, scores, n_eff

    def ranks(self, X, targets, exclude=None):
        """``(ranks, scores)``: int32 and float64 arrays with one entry per stored entry of
        ``targets`` (B, C; pattern only), in the order of its canonical CSR form -- rows in order,
        candidate ids ascending within a row, duplicates merged: the ``T`` of
        ``check_rank_lists(B, C, targets)``.  ``ranks`` is the number of candidates outside
        ``exclude`` that beat the target under (score descending, index ascending), 0-based, the
        row's other targets counted like any candidate; ``scores`` equals ``scores(X)[b, t]`` bit
        for bit.  Exact; at most 64 targets per row; -1 for a target whose score is not finite."""
        _, ranks, scores, _ = self._rank_eval(X, targets, exclude)
        return ranks, scores

    def evaluate(self, X, targets, exclude=None, ks=(10,)):
        """Full-catalogue metrics of the held-out ``targets`` with ``exclude`` left out:
        ``metrics_from_ranks`` on the exact ranks -- ``recall@k``, ``ndcg@k``, ``hit@k`` per ``k``
        in ``ks``, ``mrr``, ``auc`` (means over the rows that have a target), ``n_rows_scored``
        and the per-row arrays under ``"per_row"``."""
        ks = _check_ks(ks)
        T, ranks, _, n_eff = self._rank_eval(X, targets, exclude)
        return metrics_from_ranks(T.indptr, ranks, n_eff, ks)

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

    def rank_metrics(self, X, Z, targets, exclude=None, ks=(10,)):
        """One-shot ``ranker(Z).evaluate(X, targets, exclude, ks)``."""
        _check_ks(ks)
        Xa, Za = _prepare(self, X, Z)
        check_rank_lists(Xa.shape[0], Za.shape[0], targets, exclude)
        with Ranker(self, Z) as r:
            return r.evaluate(X, targets, exclude, ks)


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
