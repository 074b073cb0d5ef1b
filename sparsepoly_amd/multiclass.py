"""One-vs-rest multiclass classification over the binary classifiers, on the device end to end.

The binary classifiers refuse multiclass targets and point to scikit-learn's metaestimator, as
the reference does.  That metaestimator fits the classes one after the other and predicts with
one device round trip per class.  ``OneVsRestClassifier`` here fits the per-class clones on ONE
device image of ``X`` (``fit_concurrently(..., targets=...)``: side by side for pcd and psgd, one
after the other for pbcd, every clone equal to its solo fit bit for bit) and predicts through a ``ModelBank``: one pass over ``X`` for all classes,
the argmax taken on the device.
"""
import numpy as np
from sklearn.base import BaseEstimator, ClassifierMixin, clone
from sklearn.preprocessing import LabelBinarizer
from sklearn.utils.multiclass import type_of_target
from sklearn.utils.validation import NotFittedError

from .base import _NO_PROBA
from .sparse_all_subsets import SparseAllSubsetsClassifier
from .sparse_factorization_machines import SparseFactorizationMachineClassifier

_NOT_MULTICLASS = ("OneVsRestClassifier takes a 1-d multiclass target; multilabel and 2-d targets "
                   "are not supported.")


class OneVsRestClassifier(ClassifierMixin, BaseEstimator):
    """One binary clone of ``estimator`` per class (a single one for two classes, as
    scikit-learn's metaestimator), class c's clone fitted on the target +1 for c and -1 otherwise.

    ``estimator``: a ``SparseFactorizationMachineClassifier`` or ``SparseAllSubsetsClassifier``.
    ``max_concurrent`` / ``devices``: as ``fit_concurrently``, except that ``solver='pbcd'`` clones
    are by default fitted one after the other (still on the one shared image): a pbcd fit that
    shares the CUs with another adds its partial sums in another order than a solo fit, and the
    members are meant to equal solo fits bit for bit; ``max_concurrent=2`` trades that for two
    fits at a time.  ``class_weight`` (a plain attribute, default ``None``): ``'balanced'`` is
    handed to the clones, each of which balances its own one-against-the-rest problem (1 : C-1 by
    construction); a dict label -> weight over the multiclass labels becomes a per-sample vector
    that multiplies into every clone's ``sample_weight``.  Fitted attributes:
    ``estimators_``, ``classes_``, ``n_features_in_``.  The bank of the fitted clones is built on
    first use and kept; ``release_device()`` drops it (pickling does too)."""

    def __init__(self, estimator, max_concurrent=None, devices=None):
        self.estimator = estimator
        self.max_concurrent = max_concurrent
        self.devices = devices

    class_weight = None

    # ------------------------------------------------------------------ fit
    def fit(self, X, y, sample_weight=None):
        from .concurrent import fit_concurrently
        from .weights import check_sample_weight, class_weight_vector

        if not isinstance(self.estimator, (SparseFactorizationMachineClassifier,
                                           SparseAllSubsetsClassifier)):
            raise TypeError("estimator must be a SparseFactorizationMachineClassifier or a "
                            "SparseAllSubsetsClassifier, got %s" % type(self.estimator).__name__)
        if isinstance(X, (list, tuple)):
            X = np.asarray(X)  # (a list X would mean one data set per clone to fit_concurrently)
        if np.ndim(y) != 1 or type_of_target(y) not in ("binary", "multiclass"):
            raise TypeError(_NOT_MULTICLASS)
        n_rows = X.shape[0] if hasattr(X, "shape") else len(X)
        if len(y) != n_rows:
            raise ValueError("y has %d entries, X has %d rows" % (len(y), n_rows))
        binarizer = LabelBinarizer(pos_label=1, neg_label=-1)
        Y = binarizer.fit_transform(y).astype(np.double)  # (n, C); (n, 1) for two classes
        if len(binarizer.classes_) < 2:
            raise ValueError("y holds a single class")
        self.release_device()
        ests = [clone(self.estimator) for _ in range(Y.shape[1])]
        cw = self.class_weight
        if cw is None:  # (clone() copies constructor parameters only)
            cw = getattr(self.estimator, "class_weight", None)
        sw = None if sample_weight is None else check_sample_weight(sample_weight, n_rows)
        if isinstance(cw, dict):
            sw = class_weight_vector(cw, y) * (1.0 if sw is None else sw)
            cw = None
        for e in ests:
            e.class_weight = cw
        max_concurrent = self.max_concurrent
        if max_concurrent is None and self.estimator.solver == "pbcd":
            max_concurrent = 1  # the whole GPU each, as a solo fit has it (see the class docstring)
        fit_concurrently(ests, X, None, max_concurrent=max_concurrent, devices=self.devices,
                         targets=[Y[:, c] for c in range(Y.shape[1])],
                         sample_weights=None if sw is None else [sw] * len(ests))
        self.estimators_ = ests
        self.classes_ = binarizer.classes_
        self.label_binarizer_ = binarizer
        self.n_features_in_ = X.shape[1] if hasattr(X, "shape") else np.shape(X)[1]
        return self

    # ------------------------------------------------------------------ device state
    def _bank(self):
        if not hasattr(self, "estimators_"):
            raise NotFittedError("Estimator not fitted.")
        bank = getattr(self, "_device_bank", None)
        if bank is None:
            from .bank import ModelBank

            bank = self._device_bank = ModelBank(self.estimators_)
        return bank

    def release_device(self):
        """Free the resident bank of the fitted clones (it is rebuilt on the next use)."""
        bank = getattr(self, "_device_bank", None)
        self._device_bank = None
        if bank is not None:
            bank.close()

    def __getstate__(self):
        state = dict(super().__getstate__())
        state.pop("_device_bank", None)  # a device handle is not picklable
        return state

    def __del__(self):
        try:
            self.release_device()
        except Exception:
            pass

    # ------------------------------------------------------------------ predict
    def decision_function(self, X):
        """(n, C): column c is class ``classes_[c]``'s clone; (n,) for two classes (positive
        means ``classes_[1]``)."""
        scores = self._bank().decision_function(X)
        return scores[:, 0] if len(self.estimators_) == 1 else scores

    def predict(self, X):
        """``classes_[argmax_c decision_function(X)]``, the argmax taken on the device (ties go
        to the lowest class index); two classes: ``decision_function(X) > 0``."""
        if not hasattr(self, "estimators_"):
            raise NotFittedError("Estimator not fitted.")
        if len(self.estimators_) == 1:
            return self.classes_[(self.decision_function(X) > 0).astype(int)]
        return self.classes_[self._bank().argmax(X)[0]]

    def predict_proba(self, X):
        """(n, C): the per-class sigmoids of the scores, normalised per row as scikit-learn's
        one-vs-rest does (host arithmetic on the bank's scores); two classes: ``[1 - p, p]``.
        ``loss='logistic'`` only."""
        if self.estimator.loss != "logistic":
            raise ValueError(_NO_PROBA)
        scores = self._bank().decision_function(X)
        Y = 1 / (1 + np.exp(-scores))
        if len(self.estimators_) == 1:
            Y = np.concatenate(((1 - Y), Y), axis=1)
        sums = Y.sum(axis=1)[:, None]
        np.divide(Y, sums, out=Y, where=sums != 0)
        return Y
