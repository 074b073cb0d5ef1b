"""Objective, sparsity and held-out loss of a live fit, evaluated on the device.

``ObjectiveMixin`` gives the estimators ``objective_terms()``, ``objective(X, y)``,
``set_validation(X_val, y_val)`` and ``validation_loss()``; ``Monitor`` is a callback object that
records them per iteration.  The numbers come from ``spfm_loss_sum``, ``spfm_objective_terms`` and
``spfm_eval_loss`` (``include/spfm.h``): the parameters never leave the device, the held-out matrix
is uploaded once per fit.  There is no CPU path: without the library or a GPU the calls raise.

The objective is what the reference's solvers minimise,

    sum_i loss(y_pred_i, y_i) + alpha/2 |w|^2 + sum_o (beta/2 |P_o|^2 + gamma Omega(P_o)),

with ``alpha, beta, gamma`` multiplied by ``n_samples`` for ``mean=True`` as the fit loops do.
``Omega`` is the reference's ``regularizer.eval`` except for ``omegacs``, where it is the value
of the prox cache (``HipEngine.objective_terms`` explains the deviation).
"""
import numpy as np
from sklearn.utils.multiclass import type_of_target
from sklearn.utils.validation import check_array, check_X_y, NotFittedError

from .engine import SpfmError

_NO_SESSION = ("%s needs a live device session: call it from a callback while fit is running, "
               "or after fit with warm_start=True (until release_device()).")


class Monitor(object):
    """Callback that records ``estimator.objective_terms()`` every ``every``-th time it is called
    (plus ``iteration``, the call index, and ``validation_loss`` when the estimator has a
    validation set and ``validation`` is true) in ``history``.  It returns None, so it never stops
    a fit.  ``needs_params = False`` tells the fit loops that the callback does not read ``P_`` /
    ``w_``: the parameters are not copied to the host for it.

    ``interactions=True`` (opt-in: one pass over the pairwise product per record,
    sparsepoly_amd/interactions.py) adds ``nnz_interactions``, the number of feature pairs with
    ``|W| > interaction_tol``; the default records are unchanged."""

    needs_params = False

    def __init__(self, every=1, validation=True, interactions=False, interaction_tol=0.0):
        self.every = max(1, int(every))
        self.validation = bool(validation)
        self.interactions = bool(interactions)
        self.interaction_tol = float(interaction_tol)
        self.history = []
        self._calls = 0

    def __call__(self, estimator):
        it = self._calls
        self._calls += 1
        if it % self.every:
            return None
        rec = dict(estimator.objective_terms())
        rec["iteration"] = it
        rec["validation_loss"] = None
        if self.validation and getattr(estimator, "_validation", None) is not None:
            rec["validation_loss"] = estimator.validation_loss()
        if self.interactions:
            rec["nnz_interactions"] = estimator.interaction_stats(self.interaction_tol)["nnz"]
        self.history.append(rec)
        return None


def callback_needs_params(callback):
    """False only for a callback that says so (``needs_params = False``, e.g. ``Monitor``)."""
    return getattr(callback, "needs_params", True) is not False


class ObjectiveMixin(object):
    """Shared by the factorization-machine and all-subsets estimators.  The estimator provides
    ``_obj_blocks()`` -> [(order_idx, degree), ...], ``_obj_scaled(n)`` -> (alpha, beta, gamma),
    ``_obj_pred_args()`` -> (degree, fit_linear, add_lower_deg2), ``_obj_has_w``,
    ``_obj_prepare(X)`` (validation + augmentation of ``predict`` input) and
    ``_obj_configure(engine)`` (-> the plug-in regularizer object, or None)."""

    _obj_has_w = True

    # ---------------------------------------------------------------- live session
    def _live_session(self, what):
        live = getattr(self, "_live", None)
        if live is None:
            # a kept warm_start session: (key, engine), key[0] = fingerprint (shape, nnz, hash)
            cached = getattr(self, "_device_session", None)
            if cached is not None:
                live = (cached[1], int(cached[0][0][0][0]))
                if getattr(live[0], "_h", None) is not None and live[0].sample_weight_set():
                    live = (live[0], live[0].sample_weight_sum())  # mean=True scales by sum(w)
        if live is None or getattr(live[0], "_h", None) is None:
            raise SpfmError(_NO_SESSION % what)
        return live

    def _terms_from(self, engine, n_samples, plugin="live"):
        blocks = self._obj_blocks()
        alpha, beta, gamma = self._obj_scaled(n_samples)
        has_pred = self.solver != "psgd"  # psgd keeps no y_pred
        loss = engine.loss_sum() if has_pred else None
        tw = engine.objective_terms(-1, 1) if self._obj_has_w else dict(l2=0.0, nnz=0)
        per = [engine.objective_terms(o, deg) for o, deg in blocks]
        omega = [t["omega"] for t in per]
        if plugin == "live":
            plugin = getattr(self, "_plugin_reg", None)
        if plugin is not None:  # a user's regularizer object: its own eval, on the host
            P, _ = engine.get_params()
            omega = [float(plugin.eval(P[o].T, deg)) for o, deg in blocks]
        rec = dict(loss=loss, l2_w=tw["l2"], l2_P=[t["l2"] for t in per], omega=omega,
                   nnz_P=[t["nnz"] for t in per],
                   active_features=[t["active_features"] for t in per],
                   active_components=[t["active_components"] for t in per], nnz_w=tw["nnz"])
        rec["objective"] = None
        if loss is not None:
            obj = loss + alpha * tw["l2"]
            for t, om in zip(per, omega):
                obj += beta * t["l2"] + gamma * om
            rec["objective"] = obj
        return rec

    def objective_terms(self):
        """Terms of the objective of the LIVE fit, from the device: dict with ``loss`` (sum over
        the training samples), ``l2_w``, ``l2_P`` / ``omega`` / ``nnz_P`` / ``active_features`` /
        ``active_components`` (lists, one entry per order of ``P_``), ``nnz_w`` and ``objective``.
        ``loss`` and ``objective`` are None for ``solver='psgd'`` (it keeps no ``y_pred``).  Valid
        from a callback while ``fit`` runs, and afterwards while a ``warm_start`` device session
        is kept; raises ``SpfmError`` otherwise."""
        engine, n = self._live_session("objective_terms()")
        return self._terms_from(engine, n)

    def validation_loss(self):
        """Sum of the loss over the validation set (``set_validation``) under the live
        parameters; valid where ``objective_terms()`` is."""
        if getattr(self, "_validation", None) is None:
            raise ValueError("validation_loss(): call set_validation(X_val, y_val) before fit.")
        engine, _ = self._live_session("validation_loss()")
        return engine.eval_loss(*self._obj_pred_args())

    # ---------------------------------------------------------------- validation set
    def set_validation(self, X_val, y_val):
        """Held-out data whose loss the fit reports (``validation_loss()``, ``validation_loss_``,
        ``Monitor``).  Not a constructor keyword: it is no part of ``get_params()``, is not
        cloned and not pickled.  ``X_val`` is validated like ``predict`` input, ``y_val`` like
        ``fit``'s targets (a classifier maps it with the binarizer fitted on the training
        labels).  ``set_validation(None, None)`` removes it."""
        if X_val is None:
            self._validation = None
            return self
        binary = hasattr(self, "decision_function")
        if binary:
            two_d = np.ndim(y_val) > 1 and np.shape(y_val)[1] >= 2
            if two_d or type_of_target(y_val) != "binary":
                from .base import _NOT_BINARY

                raise TypeError(_NOT_BINARY)
            X_val, y_val = check_X_y(X_val, y_val, dtype=np.double, accept_sparse=("csr", "csc"),
                                     multi_output=False)
        else:
            X_val, y_val = check_X_y(X_val, y_val, dtype=np.double, accept_sparse=("csr", "csc"),
                                     multi_output=False, y_numeric=True)
            y_val = np.asarray(y_val, dtype=np.double).ravel()
        self._validation = (X_val, y_val)
        if hasattr(self, "P_"):
            self._check_validation(np.shape(self.P_)[-1], augmented=True)
        return self

    def _check_validation(self, n_features, augmented=False):
        """the column count of the validation set against the training data's (``predict``'s
        ValueError)"""
        val = getattr(self, "_validation", None)
        if val is None:
            return
        nv = val[0].shape[1]
        if augmented:
            nv = self._obj_prepare(val[0][:0]).shape[1]
        if nv != n_features:
            raise ValueError("X_val has %d features, the training data has %d"
                             % (nv, n_features))

    def _upload_validation(self, engine):
        val = getattr(self, "_validation", None)
        if val is None:
            return
        Xv, yv = val
        if hasattr(self, "label_binarizer_") and hasattr(self, "decision_function"):
            yv = self.label_binarizer_.transform(yv).ravel().astype(np.double)
        engine.set_eval_data(self._obj_prepare(Xv), yv)

    # ---------------------------------------------------------------- any data
    def objective(self, X, y):
        """The dict of ``objective_terms()`` for a FITTED estimator and any data, through a fresh
        engine.  ``X, y`` are validated (and augmented) as in ``fit``; a classifier's labels go
        through the binarizer of its fit."""
        if not hasattr(self, "P_"):
            raise NotFittedError("Estimator not fitted.")
        if hasattr(self, "decision_function"):
            from .base import _validated_xy

            X, _, _ = _validated_xy(X, y, binary=True)
            y = self.label_binarizer_.transform(y).ravel().astype(np.double)
        else:
            X, y = self._check_X_y(X, y)
        X = self._obj_prepare(X, checked=True)
        engine = self._new_engine()
        try:
            engine.set_data(X, y)
            P = np.ascontiguousarray(self.P_, dtype=np.double)
            P = P[None] if P.ndim == 2 else P
            w = getattr(self, "w_", None)
            engine.set_params(P, np.zeros(P.shape[2]) if w is None else w, self.lams_)
            plugin = self._obj_configure(engine)
            if self.solver != "psgd":
                engine.init_pred(*self._obj_pred_args())
            return self._terms_from(engine, X.shape[0], plugin=plugin)
        finally:
            engine.close()

    def __getstate__(self):
        state = dict(super().__getstate__())
        for key in ("_validation", "_live"):
            state.pop(key, None)
        return state
