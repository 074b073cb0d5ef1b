"""Cross-validation of a parameter grid on one device image.

Choosing ``gamma`` / ``beta`` is the daily use of the sparse regularizers.  ``cross_validate_path``
fits one clone per (grid point, fold) side by side -- K folds are K 0/1 masks over ONE device image
and one colouring (``fit_concurrently(..., sample_weights=masks)``) -- stacks
the fitted clones into ``ModelBank``s and scores every clone on every fold in one pass over ``X``
per bank (``ModelBank.group_sums``).  Only the small (member, fold) tables
leave the device; the held-out and the training scores are read off them on the host.  With
``rank_metrics=("auc",)`` every bank makes one more pass, ``ModelBank.group_auc`` (DESIGN.md section
22): the exact ROC-AUC of every clone on its held-out fold and on the union of the other folds --
the latter is no function of per-fold values, so each clone asks for both sets of rows by name.
``"average_precision"`` and ``"ks"`` (``ModelBank.group_curve``) come from a
second walk over the same sorted scores: any subset of the three names is still ONE more pass.

``fold_ids`` and the assembly of the result (``assemble_cv``) are pure NumPy.

Out of scope: partial AUC and TPR at a fixed FPR, thresholds chosen on the training side of a fold
and scored on the held-out side, the ranker, nested cross-validation.
"""
import numpy as np

from . import _capi
from .base import SparsePolyClassifierMixin, _validated_xy
from .weights import check_sample_weight


def fold_ids(n, n_folds, shuffle=True, random_state=None, stratify=None):
    """(n,) int32 fold ids in [0, n_folds) with fold sizes that differ by at most 1; with
    ``stratify`` (n labels) the sizes differ by at most 1 within every class as well.  The rows
    (``shuffle``: in an order drawn from ``random_state``; stratified: class after class in label
    order, each shuffled on its own) are dealt to the folds in turn.  Uses no device."""
    n, K = int(n), int(n_folds)
    if K < 2:
        raise ValueError("n_folds must be >= 2, got %r" % (n_folds,))
    if n < K:
        raise ValueError("%d folds need at least as many rows, got %d" % (K, n))
    rng = np.random.RandomState(random_state) if not isinstance(
        random_state, np.random.RandomState) else random_state
    if stratify is None:
        order = rng.permutation(n) if shuffle else np.arange(n)
    else:
        labels = np.asarray(stratify).ravel()
        if labels.shape[0] != n:
            raise ValueError("stratify must hold %d labels, got %d" % (n, labels.shape[0]))
        _, inverse = np.unique(labels, return_inverse=True)
        runs = []
        for c in range(int(inverse.max()) + 1):
            at = np.flatnonzero(inverse == c)
            runs.append(rng.permutation(at) if shuffle else at)
        order = np.concatenate(runs)
    out = np.empty(n, dtype=np.int32)
    out[order] = np.arange(n) % K
    return out


def assemble_cv(tables, weight, held):
    """From the tables of a scoring pass to held-out and training scores; a pure function.
    ``tables``: dict metric -> (n_members, K), cell [m, g] the weighted sum of the metric of member
    ``m`` over the rows of fold ``g``; ``weight`` (K,) the folds' total weights; ``held`` (n_members,)
    the fold each member did not train on.  Returns dict metric -> ``(test, train)``, (n_members,)
    each: ``test[m]`` the cell of the member's own held-out fold divided by that fold's weight,
    ``train[m]`` the other folds' cells added in ascending fold order, divided by the sum (same
    order) of their weights."""
    weight = np.asarray(weight, dtype=np.double)
    held = np.asarray(held, dtype=np.intp)
    K = weight.shape[0]
    out = {}
    for name, tab in tables.items():
        tab = np.asarray(tab, dtype=np.double)
        if tab.shape != (held.shape[0], K):
            raise ValueError("table %r must be (%d, %d), got %r"
                             % (name, held.shape[0], K, tab.shape))
        at = np.arange(held.shape[0])
        test = tab[at, held] / weight[held]
        num = np.zeros(held.shape[0])
        den = np.zeros(held.shape[0])
        for g in range(K):
            other = held != g
            num[other] += tab[other, g]
            den[other] += weight[g]
        out[name] = (test, num / den)
    return out


def _kind(est):
    """what the members of one bank share, from the constructor parameters"""
    degree = getattr(est, "degree", None)
    if degree is None:
        return ("all-subsets",)
    return ("fm", degree, getattr(est, "fit_lower", None), bool(getattr(est, "fit_linear", False)))


def bank_chunks(kinds, n_components):
    """Members -> banks.  ``kinds[i]`` (hashable) and ``n_components[i]`` of member ``i``; returns
    a list of index lists: the members of one kind in grid order, cut whenever the next member
    would be the 65th of its bank or take it past 4096 stacked components.  The kinds come in the
    order of their first member."""
    by_kind = {}
    for i, kd in enumerate(kinds):
        by_kind.setdefault(kd, []).append(i)
    chunks = []
    for members in by_kind.values():
        cur, comps = [], 0
        for i in members:
            k = int(n_components[i])
            if cur and (len(cur) == _capi.BANK_MAX_MODELS
                        or comps + k > _capi.BANK_MAX_COMPONENTS):
                chunks.append(cur)
                cur, comps = [], 0
            cur.append(i)
            comps += k
        chunks.append(cur)
    return chunks


def _folds_of(cv, X, y, n, estimator, classifier):
    """(n,) int32 fold ids and K from the three forms of ``cv``"""
    if isinstance(cv, (int, np.integer)) and not isinstance(cv, bool):
        K = int(cv)
        if K < 2:
            raise ValueError("cv needs at least 2 folds, got %d" % K)
        _check_K(K)
        fold = fold_ids(n, K, shuffle=True, random_state=getattr(estimator, "random_state", None),
                        stratify=y if classifier else None)
        return fold, K
    if hasattr(cv, "split"):
        seen = np.zeros(n, dtype=np.int64)
        fold = np.zeros(n, dtype=np.int32)
        K = 0
        for _, test in cv.split(X, y):
            test = np.asarray(test, dtype=np.intp)
            np.add.at(seen, test, 1)
            fold[test] = K
            K += 1
        if (seen == 0).any():
            raise ValueError("cv: row %d is in no test set; the test sets must partition the rows"
                             % int(np.flatnonzero(seen == 0)[0]))
        if (seen > 1).any():
            raise ValueError("cv: row %d is in two test sets; the test sets must partition the "
                             "rows" % int(np.flatnonzero(seen > 1)[0]))
    else:
        f = np.asarray(cv)
        if f.shape != (n,):
            raise ValueError("cv must be an int, an (n,) array of fold ids or an object with "
                             ".split(X, y); got an array of shape %r" % (f.shape,))
        if f.dtype.kind not in "iu" and (f.dtype.kind != "f" or not np.all(np.isfinite(f))
                                         or np.any(f != np.rint(f))):
            raise ValueError("cv: fold ids must be integers")
        if f.min() < 0:
            raise ValueError("cv: fold ids must be >= 0")
        fold = f.astype(np.int32)
        K = int(fold.max()) + 1
    if K < 2:
        raise ValueError("cv needs at least 2 folds, got %d" % K)
    _check_K(K)
    return fold, K


def _check_K(K):
    if K > _capi.BANK_MAX_GROUPS:
        raise ValueError("%d folds exceed the cap of %d (SPFM_BANK_MAX_GROUPS)"
                         % (K, _capi.BANK_MAX_GROUPS))


def _clones(estimator, grid):
    """one clone per grid position (``fit_path``'s convention, checks and messages), carrying the
    instance's non-constructor settings"""
    from sklearn.base import clone

    if not grid:
        raise ValueError("cross_validate_path needs at least one parameter sequence "
                         "(e.g. gamma=[...]).")
    lengths = {len(v) for v in grid.values()}
    if len(lengths) != 1:
        raise ValueError("all parameter sequences must have the same length.")
    valid = estimator.get_params()
    for name in grid:
        if name not in valid:
            raise ValueError("%r is not a parameter of %s." % (name, type(estimator).__name__))
    params = [{name: values[i] for name, values in grid.items()} for i in range(lengths.pop())]

    def make(p):
        e = clone(estimator)
        e.set_params(**p)
        if getattr(estimator, "_validation", None) is not None:
            e._validation = estimator._validation  # set_validation: not a constructor keyword
        for name in ("class_weight", "adagrad_init"):  # class attributes, set on the instance
            if name in vars(estimator):
                setattr(e, name, vars(estimator)[name])
        return e

    return params, make


def _check_weighted_fit(est):
    """what a weighted ``fit`` refuses, before any device work"""
    from .pairwise import SparseFactorizationMachineRanker

    if isinstance(est, SparseFactorizationMachineRanker):
        raise ValueError("cross_validate_path does not take the ranker (its fit has its own "
                         "per-positive sample_weight).")
    if getattr(est, "distributed", False):
        raise ValueError("sample_weight / class_weight run on one GPU (distributed=False).")
    reg = est._get_regularizer(est.regularizer)
    builtin = getattr(est, "_is_builtin_regularizer", None)
    if builtin is not None and not builtin(reg):
        raise ValueError("sample_weight / class_weight need one of the built-in regularizers "
                         "(host-stepped epochs take no weights).")
    est._get_loss(est.loss)


RANK_METRICS = ("auc", "average_precision", "ks")


def _rank_args(rank_metrics, select, metrics, classifier, refit):
    """the checked ``rank_metrics`` (a tuple) of ``cross_validate_path``; every error is a
    ValueError"""
    if isinstance(rank_metrics, str):
        rank_metrics = (rank_metrics,)
    rank_metrics = tuple(rank_metrics)
    for m in rank_metrics:
        if not isinstance(m, str) or m not in RANK_METRICS:
            raise ValueError("unknown rank metric %r: rank_metrics must be among %s"
                             % (m, RANK_METRICS))
    if len(set(rank_metrics)) != len(rank_metrics):
        raise ValueError("rank_metrics %r name the same metric twice" % (rank_metrics,))
    if rank_metrics and not classifier:
        raise ValueError("rank_metrics need a classifier: the ROC-AUC of a regressor's targets is "
                         "not defined")
    if select is not None and select != "loss" and select not in rank_metrics:
        raise ValueError("select must be None, 'loss' or one of rank_metrics %r, got %r"
                         % (rank_metrics, select))
    if select == "loss" and "loss" not in metrics:
        raise ValueError("select='loss' picks the smallest mean test 'loss': add it to metrics")
    if refit and select not in rank_metrics and "loss" not in metrics:
        raise ValueError("refit=True picks the smallest mean test 'loss': add it to metrics")
    return rank_metrics


def _check_rank_folds(y_score, w, fold, K):
    """every held-out fold holds weight of both classes -- and with it every training complement,
    which is a union of at least one such fold"""
    pos = np.bincount(fold, weights=w * (y_score > 0), minlength=K)
    neg = np.bincount(fold, weights=w * ~(y_score > 0), minlength=K)
    for f in range(K):
        if not (pos[f] > 0 and neg[f] > 0):
            raise ValueError("rank_metrics: fold %d holds no %s weight"
                             % (f, "positive" if not pos[f] > 0 else "negative"))


class CVResult(object):
    """What ``cross_validate_path`` returns.  ``params``: the grid points; ``fold_`` (n,) the fold
    ids; ``test_[metric]`` / ``train_[metric]`` (n_params, K): column f the clone that held fold f
    out, scored on that fold / on the other folds; ``mean_test_[metric]`` / ``std_test_[metric]``
    (n_params,) over the folds; ``best_index_`` / ``best_params_``: the smallest mean test
    ``"loss"`` (ties: the lowest index; ``None`` without that metric) or, where a rank metric was
    named by ``select``, the largest mean test value of it (ties: the lowest index); ``estimators_``
    ``[p][f]`` the fitted clones or ``None``; ``best_estimator_`` (``refit=True``) fitted on all
    rows; ``info_``: ``banks``, ``passes`` over ``X`` and ``members`` per bank."""

    def __init__(self, params, fold, K, scores, estimators, info, select=None):
        self.params = params
        self.fold_ = fold
        self.n_folds_ = K
        shape = (len(params), K)
        self.test_ = {m: t.reshape(shape) for m, (t, _) in scores.items()}
        self.train_ = {m: t.reshape(shape) for m, (_, t) in scores.items()}
        self.mean_test_ = {m: t.mean(axis=1) for m, t in self.test_.items()}
        self.std_test_ = {m: t.std(axis=1) for m, t in self.test_.items()}
        self.best_index_ = self.best_params_ = None
        if select in RANK_METRICS:
            self.best_index_ = int(np.argmax(self.mean_test_[select]))  # first of the largest
            self.best_params_ = params[self.best_index_]
        elif "loss" in self.mean_test_:
            self.best_index_ = int(np.argmin(self.mean_test_["loss"]))  # first of the smallest
            self.best_params_ = params[self.best_index_]
        self.estimators_ = estimators
        self.best_estimator_ = None
        self.info_ = info


def cross_validate_path(estimator, X, y, cv=5, sample_weight=None, metrics=None, refit=False,
                        keep_estimators=True, max_concurrent=None, devices=None, rank_metrics=(),
                        select=None, **grid):
    """K-fold cross-validation of a parameter grid: ``grid`` as for ``fit_path`` (keyword ->
    sequence, all of one length).  For every grid point ``p`` and fold ``f`` a clone is fitted with
    ``sample_weight = (fold != f) * w`` -- all of them side by side over one device image per
    device -- and every clone is scored on every fold by one ``ModelBank.group_sums`` pass over
    ``X`` per bank, with the user's ``sample_weight`` (class weights train but do not score).

    ``cv``: an int (``fold_ids``, stratified for classifiers, seeded from
    ``estimator.random_state``), an (n,) array of fold ids, or an object with ``.split(X, y)``
    whose test sets partition the rows.  ``metrics``: names of ``ModelBank.group_sums``; default
    ``("loss",)``, classifiers ``("loss", "sign_error")``.  ``refit``: fit the best grid point on
    all rows.  ``rank_metrics``: names among ``("auc", "average_precision", "ks")``, classifiers
    only: ONE more pass per bank, whatever the subset (``ModelBank.group_auc`` for ``("auc",)``
    alone, else ``ModelBank.group_curve``), gives every clone's exact ROC-AUC, average precision and
    KS distance on its held-out fold (``test_[m]``) and on the union of the other folds
    (``train_[m]``), weighted by ``sample_weight``; a fold or a training complement without
    positive or without negative weight is refused.  ``"best_f1"`` is not among them: a threshold
    chosen on the held-out fold and scored on that same fold is optimistic (use
    ``operating_point`` on rows of its own).  ``select``: what ``best_index_``, ``best_params_`` and ``refit`` go by: ``None`` /
    ``"loss"`` the smallest mean test ``"loss"``, a rank metric the largest mean test value (ties:
    the lowest index).  Returns a ``CVResult``.  Every argument error, and whatever a weighted
    ``fit`` refuses (``distributed=True``, plug-in regularizer objects, the ranker), is a
    ValueError raised before any device work."""
    from .bank import ModelBank, _group_args
    from .concurrent import fit_concurrently

    _check_weighted_fit(estimator)
    params, make = _clones(estimator, grid)
    classifier = isinstance(estimator, SparsePolyClassifierMixin)
    # targets as the scoring pass sees them: the estimator's own label handling (+-1)
    y_score = _validated_xy(X, y, binary=classifier)[1]
    n = y_score.shape[0]
    w = np.ones(n) if sample_weight is None else check_sample_weight(sample_weight, n)
    fold, K = _folds_of(cv, X, y, n, estimator, classifier)
    fold_weight = np.bincount(fold, weights=w, minlength=K)
    if (fold_weight == 0).any():
        raise ValueError("fold %d has no held-out weight" % int(np.flatnonzero(fold_weight == 0)[0]))
    if metrics is None:
        metrics = ("loss", "sign_error") if classifier else ("loss",)
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    protos = [make(p) for p in params]
    for e in protos:
        _check_weighted_fit(e)
    losses = {e.loss for e in protos}
    if "loss" in metrics and len(losses) != 1:
        raise ValueError("the grid varies loss (%s): name the metrics explicitly instead of 'loss'"
                         % ", ".join(sorted(map(str, losses))))
    _group_args(n, 1, y_score, fold, K, sample_weight, metrics, lambda: next(iter(losses)))
    rank_metrics = _rank_args(rank_metrics, select, metrics, classifier, refit)
    if rank_metrics:
        _check_rank_folds(y_score, w, fold, K)

    clones = [make(p) for p in params for _ in range(K)]  # member p * K + f holds fold f out
    held = np.tile(np.arange(K), len(params))
    masks = [(fold != f) * w for f in held]
    fit_concurrently(clones, X, y, max_concurrent=max_concurrent, devices=devices,
                     sample_weights=masks)

    chunks = bank_chunks([_kind(e) for e in clones], [e.n_components for e in clones])
    tables = {m: np.zeros((len(clones), K)) for m in metrics}
    weight = None
    ranks = {m: (np.zeros(len(clones)), np.zeros(len(clones))) for m in rank_metrics}
    for members in chunks:
        with ModelBank([clones[i] for i in members]) as bank:
            tab = bank.group_sums(X, y_score, groups=fold, n_groups=K, sample_weight=sample_weight,
                                  metrics=metrics)
            if rank_metrics:  # per member: its held-out fold, and every other fold
                own = held[members][:, None] == np.arange(K)[None, :]
                kw = dict(groups=fold, n_groups=K, sample_weight=sample_weight,
                          sets=np.stack([own, ~own], axis=1))
                if rank_metrics == ("auc",):
                    rtab = bank.group_auc(X, y_score, **kw)
                else:  # the curve's walk, and the AUC's where asked, on one pass and one sort
                    rtab = bank.group_curve(X, y_score, auc="auc" in rank_metrics, **kw)
                for m in rank_metrics:
                    ranks[m][0][members] = rtab[m][:, 0]
                    ranks[m][1][members] = rtab[m][:, 1]
        weight = tab["weight"]
        for m in metrics:
            tables[m][members] = tab[m]
    info = dict(banks=len(chunks), passes=len(chunks) * (2 if rank_metrics else 1),
                members=[len(c) for c in chunks])
    estimators = [clones[p * K:(p + 1) * K] for p in range(len(params))] if keep_estimators \
        else None
    scores = assemble_cv(tables, weight, held)
    scores.update(ranks)
    result = CVResult(params, fold, K, scores, estimators, info, select)
    if refit:
        best = make(result.best_params_)
        kw = {} if sample_weight is None else {"sample_weight": sample_weight}
        result.best_estimator_ = best.fit(X, y, **kw)
    return result
