"""Row weights of a fit: validation, class weights and the replication restatement.

Pure Python and numpy -- nothing here needs the library or a device.  The semantics are those of
``spfm_set_sample_weight`` (``include/spfm.h``): every loss term becomes
``w_i * loss(yhat_i, y_i)``, so integer weights are row replication.  ``replicate_rows`` is that
restatement, in the tradition of the ``restate_*`` functions: the tests fit the CPU oracle on the
replicated matrix and compare the weighted device fit against it.

Out of scope: ``objective(X, y)``, ``set_validation`` / ``validation_loss`` and ``fold_in`` take no
weights; the ranker keeps its own per-positive ``sample_weight``.
"""
import numpy as np
import scipy.sparse as sp


def check_sample_weight(sample_weight, n_samples):
    """``sample_weight`` as a contiguous float64 vector of ``n_samples`` entries.  ValueError for
    a wrong shape, a negative or non-finite entry, or all zeros (what the library refuses with
    SPFM_ERR_INVALID, raised here before any device work)."""
    try:
        w = np.ascontiguousarray(sample_weight, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sample_weight must be numeric.")
    if w.ndim != 1 or w.shape[0] != n_samples:
        raise ValueError("sample_weight has shape %s, expected (%d,)" % (w.shape, n_samples))
    if not np.all(np.isfinite(w)):
        raise ValueError("sample_weight holds a NaN or an infinite value.")
    if np.any(w < 0):
        raise ValueError("sample_weight holds a negative value.")
    if not np.any(w > 0):
        raise ValueError("sample_weight is all zero.")
    return w


def class_weight_vector(class_weight, y):
    """One weight per sample from a ``class_weight``: ``None`` (ones), ``'balanced'``
    (``n_samples / (n_classes * count_c)``, as scikit-learn defines it) or a dict label ->
    weight (labels the dict lacks weigh 1; a key that is no label of ``y`` is a ValueError)."""
    y = np.asarray(y).ravel()
    if class_weight is None:
        return np.ones(y.shape[0], dtype=np.float64)
    classes, inverse = np.unique(y, return_inverse=True)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError("class_weight must be None, 'balanced' or a dict, got %r."
                             % (class_weight,))
        counts = np.bincount(inverse, minlength=classes.shape[0])
        per_class = y.shape[0] / (classes.shape[0] * counts.astype(np.float64))
    elif isinstance(class_weight, dict):
        per_class = np.ones(classes.shape[0], dtype=np.float64)
        for label, value in class_weight.items():
            at = np.flatnonzero(classes == label)
            if at.size == 0:
                raise ValueError("class_weight names the label %r, which y does not hold." % (label,))
            value = float(value)
            if not np.isfinite(value) or value < 0:
                raise ValueError("class_weight[%r] must be finite and >= 0." % (label,))
            per_class[at[0]] = value
    else:
        raise ValueError("class_weight must be None, 'balanced' or a dict, got %r."
                         % (class_weight,))
    return np.ascontiguousarray(per_class[inverse], dtype=np.float64)


def combine_weights(sample_weight, class_weight, y, n_samples):
    """What a ``fit(X, y, sample_weight)`` of an estimator with a ``class_weight`` trains with:
    the product of the two, validated, or ``None`` when neither is given."""
    if sample_weight is None and class_weight is None:
        return None
    w = np.ones(n_samples) if sample_weight is None else \
        check_sample_weight(sample_weight, n_samples)
    if class_weight is not None:
        w = w * class_weight_vector(class_weight, y)
    return check_sample_weight(w, n_samples)


def replicate_rows(X, y, sample_weight):
    """The replication restatement of an integer-weighted problem: row ``i`` of ``X`` (and
    ``y[i]``) repeated ``w_i`` times in place, rows of weight 0 dropped.  Returns ``(X_rep,
    y_rep)``, ``X_rep`` CSR for sparse input.  The unweighted fit on it is the weighted fit on
    ``(X, y, w)`` up to summation order."""
    y = np.asarray(y)
    w = check_sample_weight(sample_weight, y.shape[0])
    counts = np.rint(w).astype(np.int64)
    if np.any(counts != w):
        raise ValueError("replicate_rows needs integer weights.")
    rows = np.repeat(np.arange(y.shape[0]), counts)
    if sp.issparse(X):
        Xr = sp.csr_matrix(X)[rows]
        Xr.sort_indices()
        return Xr, y[rows]
    return np.asarray(X)[rows], y[rows]
