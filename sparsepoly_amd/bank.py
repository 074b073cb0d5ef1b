"""Score many fitted models in one pass over the rows of ``X``, on the device.

A regularisation path (``fit_path``), a cross-validation grid or the per-class members of a
one-vs-rest classifier are F fitted models over the same features.  Their own
``decision_function`` calls upload ``X`` F times and fetch, per stored entry, F short rows of
parameters.  A ``ModelBank`` stacks the models along the component axis into one resident image
(``spfm_bank_*``, ``include/spfm.h``): ``X`` goes up once per call, a stored
entry costs one contiguous read of ``sum_f k_f`` doubles, and what users reduce the (n, F) scores
to -- the best model per row, a loss per model, a weighted mean, per member and fold of the rows
the weighted sums of a few metrics (``group_sums``: the scoring half of cross-validation, see
``model_selection.py``), per member and set of rows the exact ROC-AUC (``group_auc``: a sort per
member on the device), average precision, the best F1 and the KS distance
with their thresholds (``group_curve``: a second walk over the same sorted scores, section 23) -- is
formed on the device, so only that leaves it.
There is no CPU path: without the library or a GPU the device calls raise.

The members are all factorization machines of one ``degree``, ``fit_lower`` and ``fit_linear``,
or all all-subsets models, over the same features; they may differ in ``n_components``.  The score
of a member does not depend on the other members or on its position: column f of a bank equals
the one-model bank of that member bit for bit.

``restate_bank_scores`` is the plain NumPy restatement, a test aid that never touches the device;
``restate_group_sums``, ``restate_group_auc`` and ``restate_group_curve`` restate the reductions
from given scores.
"""
import numpy as np
import scipy.sparse as sp

from . import _capi
from . import engine as _engine
from .ranking import _canonical, _restate_output, _spec
from .sparse_factorization_machines import _fit_device


def _members(estimators):
    """The checked members of a bank: ``(ests, specs, kind)`` with ``specs`` the ``_spec`` of each
    and ``kind = (degree or -1, fit_linear, add_lower_deg2, d')``.  Every argument error is raised
    here, before a handle exists."""
    ests = list(estimators)
    if not ests:
        raise ValueError("a ModelBank needs at least one fitted estimator")
    specs = [_spec(e) for e in ests]  # NotFittedError for an unfitted member

    def key(e, s):
        return (s[0], s[1], s[2], getattr(e, "fit_lower", None), s[3].shape[0], s[3].shape[2])

    names = ("degree", "fit_linear", "the order-2 block", "fit_lower", "the number of blocks",
             "the number of features")
    first = key(ests[0], specs[0])
    for i, (e, s) in enumerate(zip(ests, specs)):
        if (s[0] == -1) != (first[0] == -1):
            raise ValueError("member %d: factorization machines and all-subsets models cannot "
                             "share a bank" % i)
        for name, a, b in zip(names, key(e, s), first):
            if a != b:
                raise ValueError("member %d disagrees with member 0 on %s (%r against %r): the "
                                 "members of a bank share degree, fit_lower, fit_linear and the "
                                 "features" % (i, name, a, b))
    if len(ests) > _capi.BANK_MAX_MODELS:
        raise ValueError("%d models exceed the cap of %d (SPFM_BANK_MAX_MODELS); a larger bank is "
                         "refused, never split silently" % (len(ests), _capi.BANK_MAX_MODELS))
    S = sum(s[3].shape[1] for s in specs)
    if S > _capi.BANK_MAX_COMPONENTS:
        raise ValueError("%d stacked components exceed the cap of %d "
                         "(SPFM_BANK_MAX_COMPONENTS); a larger bank is refused, never split "
                         "silently" % (S, _capi.BANK_MAX_COMPONENTS))
    return ests, specs, (first[0], first[1], first[2], first[5])


def _prepare(est, X, d_model):
    """``X`` as the members see it: check_array, ``_augment``, canonical CSR -- a copy, the
    caller's arrays are never changed"""
    Xc = _canonical(X)
    aug = getattr(est, "_augment", None)
    Xa = Xc if aug is None else sp.csr_matrix(aug(Xc))
    if Xa.shape[1] != d_model:
        raise ValueError("X has %d features, the models were fitted on %d"
                         % (Xc.shape[1], d_model - (Xa.shape[1] - Xc.shape[1])))
    if Xa is not Xc:
        Xa.sort_indices()
    return Xa


class ModelBank(object):
    """F fitted estimators resident on one device handle as a stacked image.  ``device`` and
    ``precision`` default to the first member's.  ``close()`` (or leaving the ``with`` block)
    releases the handle.  Not picklable."""

    def __init__(self, estimators, device=None, precision=None):
        self._engine = None
        self.estimators, specs, (degree, lin, lower, d_model) = _members(estimators)
        first = self.estimators[0]
        if precision is None:
            precision = first.precision
        if precision not in _capi.DTYPES:
            raise ValueError("precision must be 'f32' or 'f64'")
        self._d_model = d_model
        self.n_models = len(specs)
        blocks = [(0, degree)] + ([(1, 2)] if lower else [])
        ks = [s[3].shape[1] for s in specs]
        self.koff = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
        # feature-major, stacked: block q of every member transposed and side by side
        Pt = np.empty((len(blocks), d_model, int(self.koff[-1])))
        for q, (o, _) in enumerate(blocks):
            for f, s in enumerate(specs):
                Pt[q, :, self.koff[f]:self.koff[f + 1]] = s[3][o].T
        lams = np.concatenate([s[5] for s in specs])
        w = np.stack([s[4] for s in specs], axis=1) if lin else None
        engine = _engine.HipEngine(device=_fit_device(first) if device is None else device,
                                   precision=precision)
        try:
            engine.bank_set(self.koff, [m for _, m in blocks], Pt, lams, w)
        except Exception:
            engine.close()
            raise
        self._engine = engine

    def _X(self, X):
        if self._engine is None:
            raise ValueError("this ModelBank is closed")
        return _prepare(self.estimators[0], X, self._d_model)

    def decision_function(self, X):
        """float64 (n, F): column f is member f's ``decision_function(X)`` (regressors:
        ``predict``)."""
        return self._engine.bank_scores(self._X(X))

    def argmax(self, X):
        """``(index int32, best, runner_up)``, (n,) each: per row the member with the largest
        score (ties go to the lowest index), that score and the second largest (``-inf`` for a
        one-member bank).  The scores stay on the device."""
        return self._engine.bank_argmax(self._X(X))

    def _loss_name(self, loss):
        """``loss``, or the members' common one"""
        if loss is None:
            found = {getattr(e, "loss", None) for e in self.estimators}
            if len(found) != 1:
                raise ValueError("the members have different losses (%s): say which one with "
                                 "loss=" % ", ".join(sorted(map(str, found))))
            loss = found.pop()
        if loss not in _capi.LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(_capi.LOSSES), loss))
        return loss

    def losses(self, X, y, loss=None, mean=False, sample_weight=None):
        """(F,) ``sum_i loss(score_if, y_i)`` for a shared target ``y`` (n,), or
        ``sum_i loss(score_if, y_if)`` for per-member targets ``y`` (n, F); ``mean``: divided by
        n.  ``loss`` defaults to the members' common ``loss``.  Classifier members take their
        targets already as -1 / +1.  F doubles leave the device.

        ``sample_weight`` (n,): ``sum_i w_i loss(...)``, the one-group table of ``group_sums``
        (its summation order, not this call's); ``mean`` then divides by ``sum(w)``."""
        if sample_weight is not None:
            tab = self.group_sums(X, y, sample_weight=sample_weight, metrics=("loss",), loss=loss)
            return tab["loss"][:, 0] / tab["weight"][0] if mean else tab["loss"][:, 0]
        loss = self._loss_name(loss)
        Xa = self._X(X)
        y = np.asarray(y, dtype=np.double)
        n = Xa.shape[0]
        if y.shape not in ((n,), (n, self.n_models)):
            raise ValueError("y must be (%d,) or (%d, %d), got %r"
                             % (n, n, self.n_models, y.shape))
        out = self._engine.bank_losses(Xa, y, loss)
        return out / n if mean else out

    def group_sums(self, X, y, groups=None, n_groups=None, sample_weight=None, metrics=("loss",),
                   loss=None):
        """Per member and group of rows, the weighted sum of each metric, in one pass over ``X``:
        dict metric name -> float64 (F, G), cell [f, g] ``sum_{i: groups_i = g} w_i
        metric(score_if, y_if)``, plus ``"weight"`` -> (G,), the groups' total weights
        (``np.bincount(groups, weights=w, minlength=G)``).  ``y`` (n,) or (n, F) as for ``losses``;
        ``groups`` (n,) integers in [0, G) (``None``: one group), ``n_groups`` = G (default:
        ``groups.max() + 1``, at most %d); ``sample_weight`` (n,) >= 0 (``None``: 1.0, the same
        bits as a vector of ones).  ``metrics``: up to %d distinct names among ``"loss"`` (``loss``,
        or the members' common one), ``"squared"``, ``"squared_hinge"``, ``"logistic"``,
        ``"abs_error"`` (``|score - y|``) and ``"sign_error"`` (1 where ``(score > 0) != (y >
        0)``).  A group without rows gives zeros.  Every argument error is a ValueError raised
        before the device is touched.  Only the tables leave the device."""
        Xa = self._X(X)
        ya, ga, G, wa, names, ids = _group_args(Xa.shape[0], self.n_models, y, groups, n_groups,
                                                sample_weight, metrics,
                                                lambda: self._loss_name(loss))
        tab = self._engine.bank_group_sums(Xa, ya, wa, ga, G, ids)
        out = {name: tab[q] for q, name in enumerate(names)}
        out["weight"] = np.bincount(np.zeros(Xa.shape[0], dtype=np.intp) if ga is None else ga,
                                    weights=wa, minlength=G).astype(np.double)
        return out

    def group_auc(self, X, y, groups=None, n_groups=None, sample_weight=None, sets=None):
        """Per member and set of rows the exact ROC-AUC, in one pass over ``X`` and one sort per
        member on the device: dict with ``"auc"``, ``"pos_weight"``, ``"neg_weight"``, float64
        (F, U) each, and for unweighted calls ``"pairs"`` int64 (F, U, 3): ``U2 = 2 #{s_neg <
        s_pos} + #{s_neg == s_pos}``, the positives, the negatives; ``auc = U2 / (2 n_pos
        n_neg)``.  Weighted: ``auc = sum_p w_p (sum_{q: s_q < s_p} w_q + 1/2 sum_{q: s_q = s_p}
        w_q) / (W_pos W_neg)`` over the positives ``p`` and negatives ``q`` of the set.  A row is
        positive where ``y > 0``; ``y``, ``groups``, ``n_groups`` and ``sample_weight`` as for
        ``group_sums``.  ``sets``: ``None`` (one set per group), boolean (U, G) -- set ``u`` holds
        the rows of the groups ``g`` with ``sets[u, g]``, the same for every member -- or
        (F, U, G), at most %d sets.  A set that lacks a class has ``auc`` NaN, its weights are
        reported all the same.  Every argument error is a ValueError raised before the device is
        touched.  Only the tables leave the device."""
        Xa = self._X(X)
        ya, ga, G, wa, _, _ = _group_args(Xa.shape[0], self.n_models, y, groups, n_groups,
                                          sample_weight, ("sign_error",), None)
        masks = _set_masks(sets, self.n_models, G)
        tab, pairs = self._engine.bank_group_auc(Xa, ya, wa, ga, G, masks)
        out = {"auc": tab[:, :, 0], "pos_weight": tab[:, :, 1], "neg_weight": tab[:, :, 2]}
        if pairs is not None:
            out["pairs"] = pairs
        return out

    def group_curve(self, X, y, groups=None, n_groups=None, sample_weight=None, sets=None,
                    auc=False):
        """Per member and set of rows the average precision, the best F1 and the KS distance of
        the scores, with the thresholds of the two maxima, in one pass over ``X`` and one sort per
        member on the device.  The arguments are ``group_auc``'s.  Going through a member's tie
        runs from the highest score down, with ``TP`` / ``FP`` the positive / negative weight of
        all runs down to and including a run and ``Prun`` its own positive weight, over the runs
        that hold weight of the set: ``average_precision = sum Prun TP / (TP + FP) / W_pos``,
        ``best_f1 = max 2 TP / (TP + FP + W_pos)``, ``ks = max |TP / W_pos - FP / W_neg|``; of
        several runs that reach a maximum the highest score wins.  Returns a dict of float64
        (F, U) arrays: ``"average_precision"``, ``"pos_weight"``, ``"neg_weight"``; ``"best_f1"``,
        ``"f1_threshold"``, ``"f1_tp"``, ``"f1_fp"``; ``"ks"``, ``"ks_threshold"``, ``"ks_tp"``,
        ``"ks_fp"``.  A threshold is the run's score (a zero as ``+0.0``): predict positive where
        ``decision_function >= threshold``.  Unweighted the maxima are chosen by exact integer
        comparison and ``"counts"``, int64 (F, U, 6), holds ``n_pos, n_neg, f1_tp, f1_fp, ks_tp,
        ks_fp``.  ``auc=True`` adds ``"auc"`` and, unweighted, ``"pairs"`` -- the very values of
        ``group_auc`` -- from the same pass and sorts.  ``average_precision`` and ``best_f1`` are
        NaN without positive weight (1.0 without negative weight), ``ks`` without either; a NaN
        value has a NaN threshold and ``tp = fp = 0``.  Every argument error is a ValueError raised
        before the device is touched.  Only the tables leave the device."""
        Xa = self._X(X)
        ya, ga, G, wa, _, _ = _group_args(Xa.shape[0], self.n_models, y, groups, n_groups,
                                          sample_weight, ("sign_error",), None)
        masks = _set_masks(sets, self.n_models, G)
        tab, counts, auc_tab, pairs = self._engine.bank_group_curve(Xa, ya, wa, ga, G, masks,
                                                                    auc=bool(auc))
        out = {name: tab[:, :, k] for k, name in enumerate(CURVE_FIELDS)}
        if counts is not None:
            out["counts"] = counts
        if auc_tab is not None:
            out["auc"] = auc_tab[:, :, 0]
        if pairs is not None:
            out["pairs"] = pairs
        return out

    def mean(self, X, weights=None):
        """(n,) ``sum_f weights[f] score_if``, the weights applied in member order; default
        ``1 / F``."""
        if weights is not None:
            weights = np.asarray(weights, dtype=np.double)
            if weights.shape != (self.n_models,):
                raise ValueError("weights must be (%d,), got %r"
                                 % (self.n_models, weights.shape))
        return self._engine.bank_mean(self._X(X), weights)

    def set_partition(self, slab_nnz=0):
        """Stored entries per slab of the following calls (0: the default).  No bit of a score,
        an argmax or a mean depends on it; a loss sum is reproducible for one slab size."""
        self._engine.bank_set_partition(slab_nnz)

    def info(self):
        """dict: ``slabs`` and ``launches`` of the last call, ``resident_bytes`` of the image,
        ``S`` its stacked components, ``n_models``."""
        return dict(self._engine.bank_info(), n_models=self.n_models)

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
        raise TypeError("a ModelBank holds a device handle and cannot be pickled")


ModelBank.group_sums.__doc__ %= (_capi.BANK_MAX_GROUPS, _capi.BANK_MAX_METRICS)
ModelBank.group_auc.__doc__ %= (_capi.BANK_MAX_SETS,)

METRICS = ("loss",) + tuple(sorted(_capi.BANK_METRICS))
# the SPFM_BANK_CURVE_VALUES values of one (member, set) of spfm_bank_group_curve, in its order
CURVE_FIELDS = ("average_precision", "best_f1", "f1_threshold", "f1_tp", "f1_fp", "ks",
                "ks_threshold", "ks_tp", "ks_fp", "pos_weight", "neg_weight")


def _group_args(n, F, y, groups, n_groups, sample_weight, metrics, default_loss):
    """The checked arguments of ``group_sums``: ``(y, groups int32 or None, G, weights or None,
    the metrics' names as given, their library names)``.  Every error is a ValueError; nothing
    here needs the library.  ``default_loss()`` resolves ``"loss"``."""
    y = np.asarray(y, dtype=np.double)
    if y.shape not in ((n,), (n, F)):
        raise ValueError("y must be (%d,) or (%d, %d), got %r" % (n, n, F, y.shape))
    if isinstance(metrics, str):
        metrics = (metrics,)
    names = list(metrics)
    if not names:
        raise ValueError("metrics must name at least one of %s" % (METRICS,))
    ids = []
    for m in names:
        if not isinstance(m, str) or m not in METRICS:
            raise ValueError("unknown metric %r: metrics must be among %s" % (m, METRICS))
        ids.append(default_loss() if m == "loss" else m)
    if len(set(ids)) != len(ids):
        raise ValueError("metrics %r name the same metric twice" % (names,))
    if len(ids) > _capi.BANK_MAX_METRICS:
        raise ValueError("%d metrics exceed the cap of %d (SPFM_BANK_MAX_METRICS); a longer list "
                         "is refused, never split silently" % (len(ids), _capi.BANK_MAX_METRICS))
    ga = None
    if groups is not None:
        g = np.asarray(groups)
        if g.shape != (n,):
            raise ValueError("groups must be (%d,), got %r" % (n, g.shape))
        if g.dtype.kind not in "iu":
            if g.dtype.kind != "f" or not np.all(np.isfinite(g)) or np.any(g != np.rint(g)):
                raise ValueError("groups must hold integers")
        if g.size and g.min() < 0:
            raise ValueError("groups holds a negative id")
        top = int(g.max()) + 1 if g.size else 1
        if n_groups is None:
            n_groups = top
        elif top > int(n_groups):
            raise ValueError("groups holds the id %d, n_groups is %d" % (top - 1, int(n_groups)))
    elif n_groups is None:
        n_groups = 1
    if int(n_groups) != n_groups or int(n_groups) < 1:
        raise ValueError("n_groups must be an integer >= 1, got %r" % (n_groups,))
    G = int(n_groups)
    if G > _capi.BANK_MAX_GROUPS:
        raise ValueError("%d groups exceed the cap of %d (SPFM_BANK_MAX_GROUPS); a larger table is "
                         "refused, never split silently" % (G, _capi.BANK_MAX_GROUPS))
    if groups is not None:
        ga = np.ascontiguousarray(g, dtype=np.int32)
    wa = None
    if sample_weight is not None:
        try:
            wa = np.ascontiguousarray(sample_weight, dtype=np.double)
        except (TypeError, ValueError):
            raise ValueError("sample_weight must be numeric.")
        if wa.shape != (n,):
            raise ValueError("sample_weight has shape %s, expected (%d,)" % (wa.shape, n))
        if not np.all(np.isfinite(wa)):
            raise ValueError("sample_weight holds a NaN or an infinite value.")
        if np.any(wa < 0):
            raise ValueError("sample_weight holds a negative value.")
    return y, ga, G, wa, names, ids


def _sets_array(sets, F, G):
    """``sets`` of ``group_auc`` as boolean (F, U, G); ``None``: one set per group.  Every error is
    a ValueError; nothing here needs the library."""
    if sets is None:
        return np.broadcast_to(np.eye(G, dtype=bool), (F, G, G))
    a = np.asarray(sets)
    if a.dtype != bool:
        if a.dtype.kind not in "iuf" or np.any((a != 0) & (a != 1)):
            raise ValueError("sets must be boolean")
        a = a.astype(bool)
    if a.ndim == 2:
        a = np.broadcast_to(a, (F,) + a.shape)
    if a.ndim != 3 or a.shape[0] != F or a.shape[2] != G:
        raise ValueError("sets must be (U, %d) or (%d, U, %d) for %d groups and %d members, got %r"
                         % (G, F, G, G, F, np.shape(sets)))
    if a.shape[1] < 1:
        raise ValueError("sets must name at least one set")
    if a.shape[1] > _capi.BANK_MAX_SETS:
        raise ValueError("%d sets exceed the cap of %d (SPFM_BANK_MAX_SETS); a larger table is "
                         "refused, never split silently" % (a.shape[1], _capi.BANK_MAX_SETS))
    return a


def _set_masks(sets, F, G):
    """uint32 (F, U) bitmasks over the groups, or ``None`` for ``sets=None``"""
    if sets is None:
        return None
    a = _sets_array(sets, F, G)
    bits = np.left_shift(np.uint64(1), np.arange(G, dtype=np.uint64))
    return (a.astype(np.uint64) * bits).sum(axis=2).astype(np.uint32)


# ------------------------------------------------------------------ NumPy restatement (test aid)
def restate_bank_scores(estimators, X, wide=False):
    """Test aid, NumPy only, never touches the device: the (n, F) scores, column f what
    ``_get_output`` of member f computes on the dense rows of the checked, augmented, canonical
    ``X`` -- each column from that member's parameters alone.  ``wide``: in ``np.longdouble``.
    Dense (n, k, d) intermediates: small shapes only."""
    ests, specs, (degree, lin, lower, d_model) = _members(estimators)
    dtype = np.longdouble if wide else np.double
    Xa = _prepare(ests[0], X, d_model)
    V = np.asarray(Xa.todense(), dtype=dtype)
    used = np.flatnonzero((V != 0).any(axis=0))  # the other columns add exact zeros
    out = np.zeros((V.shape[0], len(ests)), dtype=dtype)
    for f, (_, _, _, P, w, lams) in enumerate(specs):
        out[:, f] = _restate_output(V[:, used], degree, lin, lower, P[:, :, used], w[used], lams,
                                    dtype)
    return out


def _metric(name, p, y, dtype):
    """one metric of (score, target), elementwise, by the project's piecewise definitions
    (``loss_dev`` of the device code; ``loss.py``)"""
    p, y = np.asarray(p, dtype=dtype), np.asarray(y, dtype=dtype)
    if name == "squared":
        return 0.5 * (p - y) ** 2
    if name == "squared_hinge":
        return np.maximum(1 - p * y, 0) ** 2
    if name == "logistic":
        z = p * y
        zc = np.clip(z, -18, 18)
        return np.where(z > 18, np.exp(-z), np.where(z < -18, -z, np.log1p(np.exp(-zc))))
    if name == "abs_error":
        return np.abs(p - y)
    if name == "sign_error":
        return ((p > 0) != (y > 0)).astype(dtype)
    raise ValueError("unknown metric %r" % (name,))


def restate_group_sums(scores, y, w, groups, G, metrics, wide=False):
    """Test aid, NumPy only, never touches the device: what ``group_sums`` sums, from given
    ``scores`` (n, F).  ``y`` (n,) or (n, F); ``w`` (n,) or ``None`` (ones); ``groups`` (n,) or
    ``None`` (all 0); ``metrics`` library names (``"squared"`` ..., not ``"loss"``).  Returns
    (Q, F, G), cell [q, f, g] ``sum_{i: groups_i = g} w_i metric_q(scores_if, y_if)``; ``wide``: in
    ``np.longdouble``."""
    dtype = np.longdouble if wide else np.double
    scores = np.asarray(scores, dtype=dtype)
    n, F = scores.shape
    y = np.asarray(y, dtype=dtype)
    y2 = y[:, None] if y.ndim == 1 else y
    w = np.ones(n, dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
    groups = np.zeros(n, dtype=np.intp) if groups is None else np.asarray(groups, dtype=np.intp)
    out = np.zeros((len(metrics), F, G), dtype=dtype)
    for q, name in enumerate(metrics):
        terms = w[:, None] * _metric(name, scores, y2, dtype)
        for g in range(G):
            out[q, :, g] = terms[groups == g].sum(axis=0)
    return out


def restate_group_auc(scores, y, w, groups, G, sets, wide=False):
    """Test aid, NumPy only, never touches the device: what ``group_auc`` gives, from given
    ``scores`` (n, F).  ``y`` (n,) or (n, F), positive where ``> 0``; ``w`` (n,) or ``None``;
    ``groups`` (n,) or ``None`` (all 0); ``sets`` as for ``group_auc``.  Returns the same dict.
    Unweighted (``w`` ``None``) the pairs are counted in Python integers; weighted the sums run in
    double, or in ``np.longdouble`` with ``wide``.  Per positive the negatives below it and those
    tied with it are read off the sorted negatives: ``w_p (C[lo] + C[hi]) / 2`` with ``C`` the
    running weights of the negatives -- every addend is non-negative, there is no subtraction."""
    dtype = np.longdouble if wide else np.double
    scores = np.asarray(scores, dtype=np.double) + 0.0  # (-0.0 + 0.0 = +0.0: one zero)
    n, F = scores.shape
    y = np.asarray(y, dtype=np.double)
    pos_all = np.broadcast_to((y[:, None] if y.ndim == 1 else y) > 0, (n, F))
    groups = np.zeros(n, dtype=np.intp) if groups is None else np.asarray(groups, dtype=np.intp)
    S = _sets_array(sets, F, G)
    U = S.shape[1]
    auc = np.full((F, U), np.nan)
    wpos = np.zeros((F, U), dtype=dtype)
    wneg = np.zeros((F, U), dtype=dtype)
    pairs = np.zeros((F, U, 3), dtype=np.int64)
    for f in range(F):
        for u in range(U):
            rows = S[f, u][groups]
            p = rows & pos_all[:, f]
            q = rows & ~pos_all[:, f]
            order = np.argsort(scores[q, f], kind="stable")
            sq = scores[q, f][order]
            lo = np.searchsorted(sq, scores[p, f], side="left")
            hi = np.searchsorted(sq, scores[p, f], side="right")
            if w is None:
                u2, npos, nneg = int(lo.sum()) + int(hi.sum()), int(p.sum()), int(q.sum())
                pairs[f, u] = (u2, npos, nneg)
                wpos[f, u], wneg[f, u] = npos, nneg
                if npos * nneg:
                    auc[f, u] = float(u2) / (2.0 * float(npos) * float(nneg))
                continue
            wv = np.asarray(w, dtype=dtype)
            C = np.concatenate([np.zeros(1, dtype=dtype), np.cumsum(wv[q][order], dtype=dtype)])
            num = (wv[p] * (C[lo] + C[hi])).sum(dtype=dtype) / 2
            wpos[f, u] = wv[p].sum(dtype=dtype)
            wneg[f, u] = C[-1]
            if wpos[f, u] * wneg[f, u] > 0:
                auc[f, u] = num / (wpos[f, u] * wneg[f, u])
    out = {"auc": auc, "pos_weight": wpos.astype(np.double), "neg_weight": wneg.astype(np.double)}
    if w is None:
        out["pairs"] = pairs
    return out


def restate_group_curve(scores, y, w, groups, G, sets, wide=False):
    """Test aid, NumPy only, never touches the device: what ``group_curve`` gives (without
    ``auc``), from given ``scores`` (n, F).  The arguments are ``restate_group_auc``'s.  The rows of
    a set that carry weight are gathered into tie runs from the highest score down; ``TP`` / ``FP``
    are running sums over the runs.  Unweighted (``w`` ``None``) everything is counted and compared
    in Python integers: F1 by cross-multiplication, KS by ``|TP n_neg - FP n_pos|``, a later run
    replacing the held one only when strictly greater.  Weighted the quotients ``2 TP / ((TP + FP)
    + W_pos)`` and ``|TP / W_pos - FP / W_neg|`` are compared in double, or in ``np.longdouble``
    with ``wide``; ``np.argmax`` keeps the first, the highest score.  The winning ``ks`` is reported
    as ``|TP W_neg - FP W_pos| / (W_pos W_neg)``, the integer form, so that integer weights give
    the bits of replicated rows."""
    dtype = np.longdouble if wide else np.double
    scores = np.asarray(scores, dtype=np.double) + 0.0  # (-0.0 + 0.0 = +0.0: one zero)
    n, F = scores.shape
    y = np.asarray(y, dtype=np.double)
    pos_all = np.broadcast_to((y[:, None] if y.ndim == 1 else y) > 0, (n, F))
    groups = np.zeros(n, dtype=np.intp) if groups is None else np.asarray(groups, dtype=np.intp)
    S = _sets_array(sets, F, G)
    U = S.shape[1]
    out = {name: np.zeros((F, U)) for name in CURVE_FIELDS}
    for name in ("average_precision", "best_f1", "f1_threshold", "ks", "ks_threshold"):
        out[name][:] = np.nan
    counts = np.zeros((F, U, 6), dtype=np.int64)
    wv = None if w is None else np.asarray(w, dtype=dtype)
    for f in range(F):
        for u in range(U):
            rows = S[f, u][groups]
            if wv is not None:
                rows = rows & (wv > 0)  # a row of weight 0 is the same as an absent row
            if not rows.any():
                continue
            s = scores[rows, f]
            pos = pos_all[rows, f]
            thr, inv = np.unique(-s, return_inverse=True)  # ascending in -s: the top run first
            thr = -thr + 0.0
            inv = inv.ravel()
            R = thr.shape[0]
            cell = {}
            if wv is None:
                prun = np.bincount(inv, weights=pos, minlength=R).astype(np.int64).tolist()
                nrun = np.bincount(inv, weights=~pos, minlength=R).astype(np.int64).tolist()
                npos, nneg = sum(prun), sum(nrun)
                tp = fp = 0
                ap = 0.0
                f1 = ks = None  # (tp, fp, run) held; ks with its value in front
                for r in range(R):
                    tp += prun[r]
                    fp += nrun[r]
                    ap += float(prun[r]) * (float(tp) / float(tp + fp))
                    if f1 is None or tp * (f1[0] + f1[1] + npos) > f1[0] * (tp + fp + npos):
                        f1 = (tp, fp, r)
                    v = abs(tp * nneg - fp * npos)
                    if ks is None or v > ks[0]:
                        ks = (v, tp, fp, r)
                cell["pos_weight"], cell["neg_weight"] = npos, nneg
                counts[f, u, :2] = (npos, nneg)
                if npos > 0:
                    cell["average_precision"] = ap / float(npos)
                    cell["best_f1"] = float(2 * f1[0]) / float(f1[0] + f1[1] + npos)
                    cell["f1_threshold"], cell["f1_tp"], cell["f1_fp"] = thr[f1[2]], f1[0], f1[1]
                    counts[f, u, 2:4] = f1[:2]
                if npos > 0 and nneg > 0:
                    cell["ks"] = float(ks[0]) / (float(npos) * float(nneg))
                    cell["ks_threshold"], cell["ks_tp"], cell["ks_fp"] = thr[ks[3]], ks[1], ks[2]
                    counts[f, u, 4:6] = ks[1:3]
            else:
                ws = wv[rows]
                prun = np.zeros(R, dtype=dtype)
                nrun = np.zeros(R, dtype=dtype)
                np.add.at(prun, inv[pos], ws[pos])
                np.add.at(nrun, inv[~pos], ws[~pos])
                tp, fp = np.cumsum(prun, dtype=dtype), np.cumsum(nrun, dtype=dtype)
                wpos, wneg = tp[-1], fp[-1]
                cell["pos_weight"], cell["neg_weight"] = wpos, wneg
                if wpos > 0:
                    # (cumsum adds one after the other, as the integer loop above does)
                    cell["average_precision"] = np.cumsum(prun * (tp / (tp + fp)),
                                                          dtype=dtype)[-1] / wpos
                    val = 2 * tp / ((tp + fp) + wpos)
                    r = int(np.argmax(val))
                    cell["best_f1"], cell["f1_threshold"] = val[r], thr[r]
                    cell["f1_tp"], cell["f1_fp"] = tp[r], fp[r]
                if wpos > 0 and wneg > 0:
                    val = np.abs(tp / wpos - fp / wneg)
                    r = int(np.argmax(val))
                    # chosen by the quotients, reported in the integer form
                    cell["ks"] = abs(tp[r] * wneg - fp[r] * wpos) / (wpos * wneg)
                    cell["ks_threshold"] = thr[r]
                    cell["ks_tp"], cell["ks_fp"] = tp[r], fp[r]
            for name, v in cell.items():
                out[name][f, u] = float(v)
    if w is None:
        out["counts"] = counts
    return out
