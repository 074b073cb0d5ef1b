"""Which feature pairs a fitted model kept, evaluated on the device.

For a block ``P_o`` (k, d) with signs ``lams`` the pairwise weights are
``W = P_o^T diag(lams) P_o`` over ``j < j'`` (the diagonal is no part of the model).  ``W[j, j']``
is the coefficient of ``x_j x_j'`` for the degree-2 block of a factorization machine (``P_[0]``
for ``degree=2``, the explicit lower block otherwise) and for ``P_`` of an all-subsets model.  The
reference's example notebook forms ``np.dot(P, P.T)`` and tests it against zero; at 10^5..10^6
features that matrix cannot be formed.  Here it never is: ``spfm_interaction_*``
(``include/spfm.h``) compact the active features and consume the tiles of
the product in registers.  There is no CPU path: without the library or a GPU the calls raise.

``InteractionMixin`` gives the estimators ``interaction_stats``, ``top_interactions``,
``interactions``, ``interaction_block`` and ``interaction_values``; ``support_recovery`` and
``estimation_error`` restate the notebook's metrics without a d x d array.

Per feature: ``interaction_degrees`` gives every feature its number of partners, their total and
largest weight and the strongest partner; ``top_partners`` gives the ``K`` strongest partners of
every feature (or of some), optionally among a range of features; ``partner_graph`` is that table
as a sparse kNN graph (``spfm_interaction_degrees`` / ``_partners``).  The
full square of ``W`` is walked in registers and never stored.  ``restate_partners`` and
``restate_degrees`` restate both on a dense ``W`` in NumPy, for tests.

Third order: ``T[a, j, l] = sum_s lams_s p_sa p_sj p_sl`` over ``a < j < l`` is the coefficient of
``x_a x_j x_l`` for the degree-3 block of a factorization machine (``P_[0]`` for ``degree=3``, the
explicit lower block of a higher degree) and for an all-subsets model.  ``triple_stats``,
``top_triples``, ``triples`` and ``triple_values`` (``spfm_interaction3_*``, DESIGN.md section
14a) never store ``T`` either; ``support_recovery3`` is ``support_recovery`` for a true support
of triples.
"""
import contextlib

import numpy as np
import scipy.sparse as sp
from sklearn.utils.validation import NotFittedError

_NO_DEGREE2 = ("%s: the model has no degree-2 block (degree=%d without fit_lower='explicit'); "
               "pairwise interaction weights are defined for degree=2, for the explicit lower "
               "block of a higher degree, and for all-subsets models.")
_PARTNERS_BY = ("abs", "positive", "negative")
_PARTNERS_MAX_K = 128  # SPFM_INTERACTION_MAX_K

_NO_DEGREE3 = ("%s: the model has no degree-3 block (degree=%d%s); third-order interaction weights "
               "are defined for degree=3, for the explicit lower block of a higher degree "
               "(fit_lower='explicit'), and for all-subsets models.")


class InteractionMixin(object):
    """Shared by the factorization-machine and all-subsets estimators (next to ``ObjectiveMixin``).

    Session rule.  Inside ``fit`` (from a callback) and afterwards while a ``warm_start`` device
    session is kept, the methods read that session's LIVE parameters: no parameter is copied.
    Under ``solver='pbcd'`` the fit loops do not refresh ``P_`` for callbacks, so a mid-fit call
    sees the live block, not the stale ``P_``.  Otherwise a fresh engine receives ``P_`` /
    ``lams_`` (``set_params`` only: no data, no configuration) and is closed afterwards.

    ``include_augmented``: with ``fit_lower='augment'`` the stored block has dummy columns after
    the ``n_features`` real ones; they are left out unless this is true (the first dummy is then
    feature ``n_features``).  Several ranks: parameters are replicated, every rank answers
    locally."""

    # ---------------------------------------------------------------- which block
    def _block_spec(self, what, deg):
        """(order index of the degree-``deg`` block, number of augmented dummy columns)"""
        if not hasattr(self, "P_"):
            raise NotFittedError("Estimator not fitted.")
        degree = getattr(self, "degree", None)
        if degree is None:  # all-subsets: one block, never augmented
            return 0, 0
        explicit = self.fit_lower == "explicit"
        if degree < deg or (degree > deg and not explicit):
            if deg == 2:
                raise ValueError(_NO_DEGREE2 % (what, degree))
            raise ValueError(_NO_DEGREE3 % (
                what, degree, "" if degree < 3 else " without fit_lower='explicit'"))
        n_dummy = 0
        if self.fit_lower == "augment":
            n_dummy = max(0, degree - (2 if self.fit_linear else 1))
        return degree - deg, n_dummy  # order degree - deg holds degree deg

    def _interaction_block_spec(self, what):
        return self._block_spec(what, 2)

    def _interaction3_block_spec(self, what):
        return self._block_spec(what, 3)

    @contextlib.contextmanager
    def _interaction_session(self, what, include_augmented, order=2):
        """-> (engine, order index, number of features in view)"""
        order_idx, n_dummy = self._block_spec(what, order)
        live = getattr(self, "_live", None)
        if live is None:
            cached = getattr(self, "_device_session", None)
            if cached is not None:
                live = (cached[1], None)
        fresh = live is None or getattr(live[0], "_h", None) is None
        if fresh:
            engine = self._new_engine()
            P = np.ascontiguousarray(self.P_, dtype=np.double)
            P = P[None] if P.ndim == 2 else P
            w = getattr(self, "w_", None)
            engine.set_params(P, np.zeros(P.shape[2]) if w is None else w, self.lams_)
        else:
            engine = live[0]
        d_view = engine.d if include_augmented else engine.d - n_dummy
        try:
            yield engine, order_idx, d_view
        finally:
            if fresh:
                engine.close()

    @staticmethod
    def _interaction_ids(ids, d_view, name):
        ids = np.asarray(ids)
        if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
            raise ValueError("%s must be a 1-d array of feature ids" % name)
        if ids.size and (ids.min() < 0 or ids.max() >= d_view):
            raise ValueError("%s: feature id out of range [0, %d)" % (name, d_view))
        return ids.astype(np.int32)

    # ---------------------------------------------------------------- the methods
    def interaction_stats(self, tol=0.0, include_augmented=False):
        """dict ``nnz`` (pairs ``j < j'`` with ``|W| > tol``; ``tol = 0``: ``W != 0``),
        ``active_features``, ``sum_sq``, ``sum_abs``, ``max_abs`` of the pairwise weights."""
        with self._interaction_session("interaction_stats()", include_augmented) as (eng, o, dv):
            return eng.interaction_stats(o, tol, n_features=dv)

    def top_interactions(self, K, include_augmented=False):
        """``(rows, cols, vals)`` of the ``K`` pairs of largest ``|W|`` among ``W != 0``
        (``rows < cols``), ordered by ``|W|`` descending, then row, then column; fewer than ``K``
        when fewer exist."""
        with self._interaction_session("top_interactions()", include_augmented) as (eng, o, dv):
            return eng.interaction_topk(o, K, n_features=dv)

    def interactions(self, tol=0.0, max_pairs=10_000_000, include_augmented=False):
        """Every pair with ``|W| > tol`` as an upper-triangular ``scipy.sparse.coo_matrix``
        (entries sorted by row, then column).  ``ValueError`` naming the count when it exceeds
        ``max_pairs``."""
        with self._interaction_session("interactions()", include_augmented) as (eng, o, dv):
            nnz = eng.interaction_stats(o, tol, n_features=dv)["nnz"]
            if nnz > max_pairs:
                raise ValueError("interactions(): %d pairs have |W| > %g, more than max_pairs=%d"
                                 % (nnz, tol, max_pairs))
            rows, cols, vals = eng.interaction_list(o, tol, nnz, n_features=dv)
            return sp.coo_matrix((vals, (rows, cols)), shape=(dv, dv))

    def interaction_block(self, J, J2=None, include_augmented=False):
        """The dense sub-block ``W[J, J2]`` (``J2 = J`` by default; repeats allowed), 0 where
        ``J[a] == J2[b]``.  Refused above 1 GiB of result."""
        with self._interaction_session("interaction_block()", include_augmented) as (eng, o, dv):
            J = self._interaction_ids(J, dv, "J")
            J2 = J if J2 is None else self._interaction_ids(J2, dv, "J2")
            return eng.interaction_block(o, J, J2)

    def interaction_values(self, rows, cols, include_augmented=False):
        """``W[rows[q], cols[q]]`` for given pairs (either order of the two ids; 0 where they are
        equal)."""
        with self._interaction_session("interaction_values()", include_augmented) as (eng, o, dv):
            rows = self._interaction_ids(rows, dv, "rows")
            cols = self._interaction_ids(cols, dv, "cols")
            return eng.interaction_values(o, rows, cols)

    def _interaction_support_query(self, rows, cols, include_augmented=False):
        """(``interaction_stats(0)``, ``W`` at the given pairs) through ONE session: what the
        metrics below need."""
        with self._interaction_session("support query", include_augmented) as (eng, o, dv):
            rows = self._interaction_ids(rows, dv, "rows")
            cols = self._interaction_ids(cols, dv, "cols")
            return (eng.interaction_stats(o, 0.0, n_features=dv),
                    eng.interaction_values(o, rows, cols))

    # ---------------------------------------------------------------- per feature
    def _view_width(self, what, include_augmented):
        """Features in view, from the stored block alone (no device work)"""
        _, n_dummy = self._block_spec(what, 2)
        d = np.shape(self.P_)[-1]
        return d if include_augmented else d - n_dummy

    def interaction_degrees(self, tol=0.0, include_augmented=False):
        """Per feature ``j`` in view, over its partners ``j' != j``: dict of arrays ``degree``
        (int64, partners with ``|W[j, j']| > tol``; ``tol = 0``: ``W != 0``), ``sum_abs``,
        ``max_abs`` and ``strongest`` (int32, the smallest partner attaining ``max_abs``; -1 when
        ``max_abs`` is 0).  The read-out of a feature-selecting regularizer: how many partners a
        feature kept and how much weight they carry."""
        if not float(tol) >= 0.0:
            raise ValueError("interaction_degrees(): tol must be >= 0")
        with self._interaction_session("interaction_degrees()", include_augmented) as (eng, o, dv):
            return eng.interaction_degrees(o, tol, n_features=dv)

    def top_partners(self, K, features=None, among=None, by="abs", include_augmented=False):
        """``(ids (nJ, K) int32, vals (nJ, K), counts (nJ,))``: for every feature of ``features``
        (None: every feature in view; repeats allowed) its ``K`` strongest partners ``j' != j``,
        by key descending, then id ascending -- exactly.  ``among=(lo, hi)`` keeps the partners in
        ``[lo, hi)`` only (the item field of a recommender, say).  ``by``: ``"abs"`` orders by
        ``|W|`` among ``W != 0``, ``"positive"`` by ``W`` among ``W > 0``, ``"negative"`` by ``-W``
        among ``W < 0``.  ``vals`` is the signed ``W``; a row with fewer than ``K`` admissible
        partners (``counts`` of them) is padded with ``-1`` / ``0.0``.  Argument errors are raised
        before any device work."""
        dv = self._view_width("top_partners()", include_augmented)
        features, among = _check_partner_args("top_partners()", K, features, among, by, dv)
        with self._interaction_session("top_partners()", include_augmented) as (eng, o, dv):
            return eng.interaction_partners(o, features, int(K), among=among, by=by, n_features=dv)

    # ---------------------------------------------------------------- third order
    def triple_stats(self, tol=0.0, include_augmented=False):
        """dict ``nnz`` (triples ``a < j < l`` with ``|T| > tol``; ``tol = 0``: ``T != 0``),
        ``active_features``, ``sum_sq``, ``sum_abs``, ``max_abs`` of the third-order weights."""
        with self._interaction_session("triple_stats()", include_augmented, 3) as (eng, o, dv):
            return eng.interaction3_stats(o, tol, n_features=dv)

    def top_triples(self, K, include_augmented=False):
        """``(i, j, l, vals)`` of the ``K`` triples of largest ``|T|`` among ``T != 0``
        (``i < j < l``), ordered by ``|T|`` descending, then ``i``, ``j``, ``l``; fewer than ``K``
        when fewer exist."""
        with self._interaction_session("top_triples()", include_augmented, 3) as (eng, o, dv):
            return eng.interaction3_topk(o, K, n_features=dv)

    def triples(self, tol=0.0, max_triples=10_000_000, include_augmented=False):
        """Every triple with ``|T| > tol`` as arrays ``(i, j, l, vals)`` with ``i < j < l``,
        sorted by ``(i, j, l)``.  ``ValueError`` naming the count when it exceeds
        ``max_triples``."""
        with self._interaction_session("triples()", include_augmented, 3) as (eng, o, dv):
            nnz = eng.interaction3_stats(o, tol, n_features=dv)["nnz"]
            if nnz > max_triples:
                raise ValueError("triples(): %d triples have |T| > %g, more than max_triples=%d"
                                 % (nnz, tol, max_triples))
            return eng.interaction3_list(o, tol, nnz, n_features=dv)

    def triple_values(self, i, j, l, include_augmented=False):
        """``T[i[q], j[q], l[q]]`` for given triples (any order of the three ids; 0 where two of
        them are equal)."""
        with self._interaction_session("triple_values()", include_augmented, 3) as (eng, o, dv):
            i = self._interaction_ids(i, dv, "i")
            j = self._interaction_ids(j, dv, "j")
            l = self._interaction_ids(l, dv, "l")
            return eng.interaction3_values(o, i, j, l)


# ------------------------------------------------------------------ per-feature views
def _check_partner_args(what, K, features, among, by, d_view):
    """The argument errors of ``top_partners`` -> (features as int32 or None, among or None)"""
    if int(K) != K or not 1 <= int(K) <= _PARTNERS_MAX_K:
        raise ValueError("%s: K must be an integer in [1, %d]" % (what, _PARTNERS_MAX_K))
    if by not in _PARTNERS_BY:
        raise ValueError("%s: by must be one of %s" % (what, ", ".join(map(repr, _PARTNERS_BY))))
    if features is not None:
        features = InteractionMixin._interaction_ids(features, d_view, "features")
    if among is not None:
        if len(among) != 2 or int(among[0]) != among[0] or int(among[1]) != among[1]:
            raise ValueError("%s: among must be a pair of integers (lo, hi)" % what)
        lo, hi = int(among[0]), int(among[1])
        if lo < 0 or hi > d_view:
            raise ValueError("%s: among=(%d, %d) outside [0, %d]" % (what, lo, hi, d_view))
        if lo >= hi:
            raise ValueError("%s: among=(%d, %d) is empty" % (what, lo, hi))
        among = (lo, hi)
    return features, among


def partner_graph(est, K, features=None, among=None, by="abs", include_augmented=False):
    """``est.top_partners`` as a ``scipy.sparse.csr_matrix`` of shape ``(d_view, d_view)`` with at
    most ``K`` stored entries per row: row ``j`` holds the signed weights of the ``K`` strongest
    partners of feature ``j`` (the kNN graph of the features, or a similar-items table with
    ``among`` set to the item field).  Rows outside ``features`` are empty; a repeated feature
    counts once."""
    dv = est._view_width("partner_graph()", include_augmented)
    features, among = _check_partner_args("partner_graph()", K, features, among, by, dv)
    if features is not None:
        features = np.unique(features)
    ids, vals, counts = est.top_partners(K, features=features, among=among, by=by,
                                         include_augmented=include_augmented)
    rows = np.arange(dv, dtype=np.int64) if features is None else features.astype(np.int64)
    indptr = np.zeros(dv + 1, dtype=np.int64)
    indptr[rows + 1] = counts
    np.cumsum(indptr, out=indptr)
    keep = np.arange(ids.shape[1])[None, :] < np.asarray(counts)[:, None]
    return sp.csr_matrix((vals[keep], ids[keep], indptr), shape=(dv, dv))


def _dense_w(P_block, lams):
    P = np.asarray(P_block, dtype=np.double)
    if P.ndim != 2:
        raise ValueError("P_block must be a (k, d) array")
    lams = np.asarray(lams, dtype=np.double)
    return P.T @ (lams[:, None] * P)


def restate_partners(P_block, lams, K, features=None, among=None, by="abs", W=None):
    """``top_partners`` restated on the dense ``W = P_block^T diag(lams) P_block`` (or a given
    symmetric ``W``) in NumPy: a test aid, quadratic in ``d``.  Same outputs, same order (key
    descending, then id ascending), same padding."""
    W = _dense_w(P_block, lams) if W is None else np.asarray(W, dtype=np.double)
    d = W.shape[0]
    features, among = _check_partner_args("restate_partners()", K, features, among, by, d)
    J = np.arange(d) if features is None else features
    lo, hi = (0, d) if among is None else among
    K = int(K)
    ids = np.full((len(J), K), -1, dtype=np.int32)
    vals = np.zeros((len(J), K))
    counts = np.zeros(len(J), dtype=np.int32)
    cand = np.arange(lo, hi)
    for q, j in enumerate(J):
        w = W[j, lo:hi]
        key = np.abs(w) if by == "abs" else (w if by == "positive" else -w)
        ok = (key > 0) & (cand != j)
        c, kk, ww = cand[ok], key[ok], w[ok]
        order = np.lexsort((c, -kk))[:K]
        n = order.shape[0]
        ids[q, :n], vals[q, :n], counts[q] = c[order], ww[order], n
    return ids, vals, counts


def restate_degrees(P_block, lams, tol=0.0, W=None):
    """``interaction_degrees`` restated on the dense ``W`` in NumPy: a test aid.  ``sum_abs`` is
    NumPy's row sum (equal to the device's for integer-valued blocks, otherwise up to the
    summation order)."""
    W = _dense_w(P_block, lams) if W is None else np.asarray(W, dtype=np.double)
    if not float(tol) >= 0.0:
        raise ValueError("restate_degrees(): tol must be >= 0")
    M = np.abs(W).copy()
    np.fill_diagonal(M, 0.0)
    mx = M.max(axis=1) if M.shape[0] else np.zeros(0)
    strongest = np.where(mx > 0, M.argmax(axis=1), -1).astype(np.int32)  # first = smallest id
    return dict(degree=(M > tol).sum(axis=1).astype(np.int64), sum_abs=M.sum(axis=1), max_abs=mx,
                strongest=strongest)


# ------------------------------------------------------------------ the notebook's metrics
def _true_support(W_true):
    """(rows, cols, values) of the non-zeros of the symmetric ``W_true`` above the diagonal"""
    if sp.issparse(W_true):
        Wt = sp.triu(sp.coo_matrix(W_true), k=1).tocoo()
        Wt.sum_duplicates()
        keep = Wt.data != 0
        rows, cols, vals = Wt.row[keep], Wt.col[keep], Wt.data[keep]
    else:
        W = np.asarray(W_true, dtype=np.double)
        if W.ndim != 2 or W.shape[0] != W.shape[1]:
            raise ValueError("W_true must be a square matrix")
        rows, cols = np.nonzero(np.triu(W, k=1))
        vals = W[rows, cols]
    order = np.lexsort((cols, rows))
    return (rows[order].astype(np.int32), cols[order].astype(np.int32),
            np.asarray(vals, dtype=np.double)[order])


def _support_metrics(nnz, tp, n_true):
    """The support metrics from ``nnz`` selected, ``tp`` of them true and ``n_true`` true ones.
    Zero divisions as in the notebook: precision is 0 when nothing is selected, the F-score is 0
    when precision + recall is 0; an empty true support gives recall 0."""
    nnz, tp = int(nnz), int(tp)
    fp = nnz - tp
    fn = int(n_true) - tp
    precision = 0.0 if tp + fp == 0 else tp / (tp + fp)
    recall = 0.0 if tp + fn == 0 else tp / (tp + fn)
    fscore = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return dict(fscore=fscore, pssr=(fp + fn) == 0, nnz=nnz, tp=tp, fp=fp, fn=fn)


def support_recovery(est, W_true, include_augmented=False):
    """The notebook's support metrics of ``est`` against a symmetric true matrix ``W_true``
    (dense or scipy-sparse), over pairs ``j < j'``: dict ``fscore``, ``pssr`` (the supports are
    equal), ``nnz`` (selected pairs), ``tp``, ``fp``, ``fn``.  ``tp`` counts the true pairs whose
    estimated weight is non-zero (``spfm_interaction_values`` on the true support), ``fp = nnz - tp``,
    ``fn = |supp| - tp``.  Zero divisions as in the notebook: precision is 0 when nothing is
    selected, the F-score is 0 when precision + recall is 0; an empty true support, which the
    notebook does not meet, gives recall 0.  No d x d array is formed."""
    rows, cols, _ = _true_support(W_true)
    stats, we = est._interaction_support_query(rows, cols, include_augmented)
    return _support_metrics(stats["nnz"], int(np.count_nonzero(we)), rows.shape[0])


def support_recovery3(est, support, include_augmented=False):
    """``support_recovery`` at third order: ``support = (i, j, l)`` are three id arrays naming the
    true triples (any order inside a triple; repeats of a triple count once, a triple with two
    equal ids is refused).  Same dict: ``fscore``, ``pssr``, ``nnz`` (selected triples), ``tp``,
    ``fp``, ``fn``, with the same zero-division rules.  One ``triple_stats(0)`` call plus one
    ``triple_values`` call on the true support; no d x d x d array is formed."""
    i, j, l = (np.asarray(a) for a in support)
    if not (i.ndim == j.ndim == l.ndim == 1 and i.shape == j.shape == l.shape):
        raise ValueError("support must be three 1-d id arrays of one length")
    t = np.sort(np.stack([i, j, l], axis=1).astype(np.int64).reshape(-1, 3), axis=1)
    if t.size and ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2])).any():
        raise ValueError("support: the three ids of a triple must differ")
    t = np.unique(t, axis=0) if t.size else t
    nnz = est.triple_stats(0.0, include_augmented=include_augmented)["nnz"]
    te = est.triple_values(t[:, 0], t[:, 1], t[:, 2], include_augmented=include_augmented)
    return _support_metrics(nnz, int(np.count_nonzero(te)), t.shape[0])


def estimation_error(est, W_true, scaling=True, include_augmented=False):
    """The notebook's estimation error, with its convention that the model's ``W`` estimates
    ``2 W_true``: ``sqrt(sum_{j<j'} (2 W_true - W)^2)``, divided by ``sqrt(sum_{j<j'} (2 W_true)^2)``
    when ``scaling``.  Evaluated as ``sum_supp (2 W_t - W_e)^2 + (sum_sq - sum_supp W_e^2)`` --
    the pairs outside the true support contribute their squares, which ``interaction_stats``
    sums on the device -- clamped at 0 before the root.  No d x d array is formed."""
    rows, cols, wt = _true_support(W_true)
    stats, we = est._interaction_support_query(rows, cols, include_augmented)
    sum_sq = stats["sum_sq"]
    err2 = float(np.sum((2.0 * wt - we) ** 2)) + (sum_sq - float(np.sum(we ** 2)))
    err = np.sqrt(max(err2, 0.0))
    if scaling:
        err /= np.sqrt(float(np.sum((2.0 * wt) ** 2)))
    return float(err)
