"""Fold in new features: the parameters of single columns of a fitted factorization machine
estimated on the device, every other parameter fixed.

A user or an item that appears after the fit (or an existing one that collected new rows) needs
its column of ``P_`` and ``w_`` now, without another fit over the whole matrix.  The ANOVA kernel
is multilinear, so with all other columns fixed the model output on a row ``i`` that stores the
target column ``j`` is affine in that column's parameters.  With ``x_i\\j`` the row without that
one entry,

    f(x_i)  = c_i + z_i . theta_j
    c_i     = f(x_i\\j)
    theta_j = ( w_j if fit_linear ;  p^{o_q}_{sj}  for the blocks q and the components s )
    z_i     = x_ij ( 1 if fit_linear ;  lams_s sum_{t=1..M_q} c_q[s][t] A^{t-1}(p^{o_q}_s, x_i\\j) )

over the blocks ``(o_q, M_q, c_q)`` of ``explain._model`` -- what ``decision_function`` sums,
including the ``fit_lower='augment'`` table.  The fold-in of column ``j`` is the unique minimiser
of the strictly convex

    F_j(theta) = sum_{i: x_ij stored} loss(c_i + z_i . theta, y_i)
                 + alpha/2 theta_w^2 + beta/2 |theta_P|^2

with at most ``n_blocks k + 1 <= 128`` unknowns, found by a damped Newton iteration, one
workgroup per column (``spfm_foldin_*``, ``include/spfm.h``).  Columns of
one call are independent because no row may store two of them: a batch of new users is one
device job.  There is no CPU path: without the library or a GPU the device calls raise.

What fold-in does not do: the sparsity regulariser ``gamma Omega`` couples the columns and is not
part of it (the ridge terms are); orders of ``P_`` that ``decision_function`` does not sum
(``fit_lower='explicit'`` at degree >= 4) are left untouched; the dummy columns of
``fit_lower='augment'`` cannot be folded in.  ``FoldInMixin`` gives the factorization-machine
estimators ``fold_in`` and ``extend_features``.  The all-subsets estimators do not have it: their
product over the whole row is affine in ``p_sj`` too, but its offsets are products, not kernels.
``restate_fold_in`` is the plain NumPy restatement, a test aid that never touches the device.
"""
import warnings

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.utils.validation import NotFittedError

from . import _capi
from .explain import _columns, _model

ARMIJO = 1e-4      # sufficient decrease of the line search (kFoldinArmijo)
HALVINGS = 40      # of one line search (kFoldinHalvings)


class FoldInResult(object):
    """What ``fold_in`` returns: ``columns`` (m), ``P`` (n_orders, k, m) and ``w`` (m) the
    estimated columns (orders outside the blocks and, without a linear term, ``w`` keep the
    estimator's values), per column ``n_rows``, ``n_iter``, ``converged``, ``grad_norm``
    (``max |grad F_j|`` at the result), ``objective_before = F_j(0)``, ``objective_after``;
    ``theta`` (m, R) holds the same numbers as solved: the linear weight, then the blocks."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "FoldInResult(columns=%r, converged=%r)" % (self.columns, self.converged)


class _Problem(object):
    """The checked arguments of one fold-in"""


def _problem(est, X, y, columns, alpha, beta, max_iter, tol, dtype=np.double):
    """Every argument error is raised here, before a handle exists.  ``columns`` count in the
    features of ``X``; ``cols`` are the same columns (the engine sees the real columns only)."""
    pr = _Problem()
    (pr.Xc, pr.blocks, pr.coef, pr.P, pr.w, pr.lams, pr.lin, base) = _model(est, X, dtype)
    n, d = pr.Xc.shape
    pr.real, pr.dummy = _columns(est, d)
    pr.offset = est.w_[pr.dummy].astype(dtype).sum() if pr.lin else dtype(0)
    pr.loss = est.loss
    if pr.loss not in _capi.LOSSES:
        raise ValueError("fold_in: loss %r is not one of %s" % (pr.loss, sorted(_capi.LOSSES)))
    pr.alpha = float(est.alpha if alpha is None else alpha)
    pr.beta = float(est.beta if beta is None else beta)
    if not (pr.beta > 0 and np.isfinite(pr.beta)):
        raise ValueError("fold_in: beta must be > 0, got %r" % (pr.beta,))
    if pr.lin and not (pr.alpha > 0 and np.isfinite(pr.alpha)):
        raise ValueError("fold_in: alpha must be > 0 with a linear term, got %r" % (pr.alpha,))
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("fold_in: max_iter must be an integer >= 1, got %r" % (max_iter,))
    pr.max_iter = int(max_iter)
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("fold_in: tol must be finite and >= 0, got %r" % (tol,))
    pr.tol = float(tol)
    cols = np.asarray(columns)
    if cols.ndim != 1 or (cols.size and not np.issubdtype(cols.dtype, np.integer)):
        raise ValueError("fold_in: columns must be a 1-d integer array")
    cols = cols.astype(np.int64)
    if cols.size and (cols.min() < 0 or cols.max() >= d):
        bad = cols[(cols < 0) | (cols >= d)][0]
        raise ValueError("fold_in: column %d outside [0, %d)" % (bad, d))
    if np.unique(cols).size != cols.size:
        u, cnt = np.unique(cols, return_counts=True)
        raise ValueError("fold_in: column %d is listed twice" % u[cnt > 1][0])
    pr.cols = cols.astype(np.int32)
    pr.k = pr.P.shape[1]
    pr.R = len(pr.blocks) * pr.k + int(pr.lin)
    if pr.R > _capi.FOLDIN_MAX_UNKNOWNS:
        raise ValueError("fold_in: %d unknowns per column exceed the cap of %d "
                         "(SPFM_FOLDIN_MAX_UNKNOWNS); a larger problem is refused, never answered "
                         "approximately" % (pr.R, _capi.FOLDIN_MAX_UNKNOWNS))
    if hasattr(est, "decision_function"):
        y = est.label_binarizer_.transform(y).ravel().astype(np.double)
    else:
        y = np.asarray(y, dtype=np.double).ravel()
    if y.shape != (n,):
        raise ValueError("fold_in: y holds %d targets, X has %d rows" % (y.shape[0], n))
    if not np.isfinite(y).all():
        raise ValueError("fold_in: y must be finite")
    pr.y = y
    # the row -> target map: a row belongs to at most one target column
    slot = np.full(d, -1, dtype=np.int64)
    slot[cols] = np.arange(cols.size)
    hit = slot[pr.Xc.indices] >= 0
    rows_of = np.repeat(np.arange(n), np.diff(pr.Xc.indptr))
    per_row = np.bincount(rows_of[hit], minlength=n)
    if (per_row > 1).any():
        i = int(np.flatnonzero(per_row > 1)[0])
        both = pr.Xc.indices[pr.Xc.indptr[i]:pr.Xc.indptr[i + 1]]
        both = both[slot[both] >= 0]
        raise ValueError("fold_in: row %d stores two target columns (%d and %d): the columns of "
                         "one call must not share a row" % (i, both[0], both[1]))
    pr.entry = np.flatnonzero(hit)                 # position in Xc.data of every target entry
    pr.row = rows_of[pr.entry]                     # its row (ascending)
    pr.owner = slot[pr.Xc.indices[pr.entry]]       # its target column's index in cols
    pr.ignored = int(n - pr.row.size)
    return pr


def _result(est, pr, theta, n_rows, n_iter, converged, grad_norm, obj0, obj1, **extra):
    stored = pr.real[pr.cols]
    P = np.array(np.asarray(est.P_, dtype=np.double)[:, :, stored])
    w = np.array(np.asarray(est.w_, dtype=np.double)[stored])
    extra["theta"] = np.asarray(theta)  # (m, R) as solved: the linear weight, then the blocks
    theta = np.asarray(theta, dtype=np.double)
    lin = int(pr.lin)
    if lin:
        w = theta[:, 0].copy()
    for q, (o, _) in enumerate(pr.blocks):
        P[o] = theta[:, lin + q * pr.k:lin + (q + 1) * pr.k].T
    return FoldInResult(columns=pr.cols.astype(np.int64), P=P, w=w,
                        n_rows=np.asarray(n_rows, dtype=np.int64),
                        n_iter=np.asarray(n_iter, dtype=np.int64),
                        converged=np.asarray(converged, dtype=bool),
                        grad_norm=np.asarray(grad_norm, dtype=np.double),
                        objective_before=np.asarray(obj0, dtype=np.double),
                        objective_after=np.asarray(obj1, dtype=np.double), **extra)


def run(engine, pr):
    """``spfm_foldin_csr`` for a checked problem on an engine that holds its parameters"""
    return engine.foldin(pr.Xc, pr.y, pr.blocks, pr.coef, pr.lin, float(pr.offset), pr.loss,
                         pr.cols, pr.alpha, pr.beta, pr.max_iter, pr.tol)


class FoldInMixin(object):
    """Shared by the factorization-machine estimators."""

    def fold_in(self, X, y, columns, alpha=None, beta=None, max_iter=50, tol=1e-8, update=False):
        """Estimate the parameters of the feature columns ``columns`` (indices into the features
        of ``X``) from the rows of ``X`` that store them, every other parameter fixed: per column
        the unique minimiser of

            sum_i loss(f(x_i), y_i) + alpha/2 w_j^2 + beta/2 sum_{orders, s} p_sj^2

        over the rows ``i`` that store ``j``, found on the device by a damped Newton iteration
        from zero (stopped at ``max |grad| <= tol max |grad at 0|`` or after ``max_iter`` steps).
        The values that ``P_`` and ``w_`` hold in the target columns are not read.  No row may
        store two target columns; rows that store none are ignored.  ``alpha`` / ``beta``:
        ``None`` means the estimator's own, unscaled -- they stand against the SUM of the loss
        over the column's rows, so a ``mean=True`` fit on ``n`` rows used ``n * beta`` in this
        form.  The sparsity regulariser ``gamma`` is not part of fold-in (it couples the
        columns); orders of ``P_`` that ``decision_function`` does not sum are left as they are.
        A classifier's ``y`` goes through ``label_binarizer_``.  Returns a ``FoldInResult``;
        a column that did not converge raises a ``ConvergenceWarning``.  ``update=True`` writes
        the columns into ``P_`` and ``w_``, so ``predict``, ``ranker(...)`` and the explain
        calls see them."""
        pr = _problem(self, X, y, columns, alpha, beta, max_iter, tol)
        engine = self._new_engine()
        try:
            engine.set_params(pr.P, pr.w, pr.lams)
            out = run(engine, pr)
            info = engine.foldin_info()
        finally:
            engine.close()
        res = _result(self, pr, out["theta"], out["n_rows"], out["n_iter"], out["converged"],
                      out["grad_norm"], out["obj0"], out["obj1"], info=info)
        if not res.converged.all():
            bad = res.columns[~res.converged]
            warnings.warn("fold_in: %d of %d columns did not converge (first: column %d, "
                          "max|grad| = %.3e). Increase max_iter."
                          % (bad.size, res.columns.size, bad[0],
                             res.grad_norm[~res.converged][0]), ConvergenceWarning)
        if update:
            stored = pr.real[pr.cols]
            self.P_ = np.array(self.P_, dtype=np.double)
            self.w_ = np.array(self.w_, dtype=np.double)
            self.P_[:, :, stored] = res.P
            if pr.lin:
                self.w_[stored] = res.w
        return res

    def extend_features(self, n_new):
        """Make room for ``n_new`` features that did not exist at fit time: zero columns are
        inserted into ``P_`` and ``w_`` after the last real column (the dummy columns of
        ``fit_lower='augment'`` stay where ``_augment`` puts them).  Returns the new features'
        indices, to be passed to ``fold_in`` with rows of the new width."""
        if not hasattr(self, "P_"):
            raise NotFittedError("Estimator not fitted.")
        if int(n_new) != n_new or n_new < 0:
            raise ValueError("extend_features: n_new must be an integer >= 0, got %r" % (n_new,))
        n_new = int(n_new)
        stored = self.P_.shape[2]
        probe = self._augment(np.zeros((1, 1)))
        d = stored - (probe.shape[1] - 1)          # real features so far
        real, _ = _columns(self, d)
        at = int(real[-1]) + 1 if d else 0
        self.P_ = np.ascontiguousarray(np.insert(self.P_, [at] * n_new, 0.0, axis=2))
        self.w_ = np.ascontiguousarray(np.insert(self.w_, [at] * n_new, 0.0))
        if hasattr(self, "adagrad_P_"):  # learning_rate='adagrad': new features start from zero
            self.adagrad_P_ = np.ascontiguousarray(
                np.insert(self.adagrad_P_, [at] * n_new, 0.0, axis=1))
            self.adagrad_w_ = np.ascontiguousarray(np.insert(self.adagrad_w_, [at] * n_new, 0.0))
        new_real, _ = _columns(self, d + n_new)
        assert (new_real[d:] == at + np.arange(n_new)).all()
        return np.arange(d, d + n_new)


# ------------------------------------------------------------------ NumPy restatement (test aid)
def loss_terms(loss, p, y):
    """``(l, l', l'')`` of the margins ``p`` in their own dtype: the losses as ``loss_dev`` has
    them and the derivative of the active branch of ``dloss_dev``"""
    one = p.dtype.type(1)
    if loss == "squared":
        return (p - y) ** 2 / 2, p - y, np.ones_like(p)
    if loss == "logistic":
        z = p * y
        zc = np.clip(z, -18, 18)
        ez, emz = np.exp(zc), np.exp(-np.minimum(np.maximum(z, -18), 745))
        hi, lo = z > 18, z < -18
        ls = np.where(hi, emz, np.where(lo, -z, np.log(one + np.exp(-zc))))
        d1 = np.where(hi, -y * emz, np.where(lo, -y, -y / (ez + one)))
        d2 = np.where(hi, y * y * emz, np.where(lo, 0 * z, y * y * ez / ((ez + one) ** 2)))
        return ls, d1, d2
    if loss == "squared_hinge":
        z = one - p * y
        on = z > 0
        return np.where(on, z * z, 0 * z), np.where(on, -2 * y * z, 0 * z), \
            np.where(on, 2 * y * y, 0 * z)
    raise ValueError("unknown loss %r" % (loss,))


def restate_design(pr, dtype=np.double, n_threads=1, chunk=2048):
    """Per target column ``(rows, Z, c)``: the rows that store it (ascending), their design rows
    (n_j, R) and offsets (n_j), by the recurrence over every row's other entries.  Rows of one
    length go through together, ``chunk`` at a time, on ``n_threads`` host threads."""
    Xc = pr.Xc
    P, w, lam = pr.P.astype(dtype), pr.w.astype(dtype), pr.lams.astype(dtype)
    coef = pr.coef.astype(dtype)
    m, lin = pr.row.size, int(pr.lin)
    Z = np.zeros((m, pr.R), dtype=dtype)
    c = np.full(m, dtype(pr.offset), dtype=dtype)
    lens = (Xc.indptr[pr.row + 1] - Xc.indptr[pr.row]) - 1
    xt = Xc.data[pr.entry].astype(dtype)
    if lin:
        Z[:, 0] = xt

    def work(task):  # rows `sel`, all with L other entries; writes its own rows of Z and c
        L, sel = task
        # positions of the other entries: the row's range without the target's position
        base = Xc.indptr[pr.row[sel]][:, None] + np.arange(L + 1)[None, :]
        keep = base != pr.entry[sel][:, None]
        pos = base[keep].reshape(sel.size, L)
        cj, xv = Xc.indices[pos], Xc.data[pos].astype(dtype)
        if lin:
            c[sel] += (w[cj] * xv).sum(axis=1)
        for q, (o, M) in enumerate(pr.blocks):
            PX = P[o][:, cj] * xv[None]                       # (k, rows, L)
            a = [np.ones(PX.shape[:2], dtype=dtype)] + [np.zeros(PX.shape[:2], dtype=dtype)
                                                        for _ in range(M)]
            for u in range(L):
                for t in range(M, 0, -1):
                    a[t] = a[t] + a[t - 1] * PX[:, :, u]
            zs = np.zeros(PX.shape[:2], dtype=dtype)
            cv = coef[q][:, 0][:, None] * a[0]
            for t in range(1, M + 1):
                zs = zs + coef[q][:, t][:, None] * a[t - 1]
                cv = cv + coef[q][:, t][:, None] * a[t]
            Z[sel, lin + q * pr.k:lin + (q + 1) * pr.k] = (xt[sel][None] * (lam[:, None] * zs)).T
            c[sel] += (lam[:, None] * cv).sum(axis=0)

    tasks = []
    for L in np.unique(lens):
        sel = np.flatnonzero(lens == L)
        tasks += [(int(L), sel[i:i + chunk]) for i in range(0, sel.size, chunk)]
    _map(work, tasks, n_threads)
    order = np.argsort(pr.owner, kind="stable")  # per column its rows, ascending
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pr.owner, minlength=pr.cols.size))])
    out = []
    for q in range(pr.cols.size):
        sel = order[ptr[q]:ptr[q + 1]]
        out.append((pr.row[sel], Z[sel], c[sel]))
    return out


def _map(fn, items, n_threads):
    if n_threads > 1 and len(items) > 1:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(n_threads) as pool:
            return list(pool.map(fn, items))
    return [fn(it) for it in items]


def _cholesky_solve(H, b):
    """``H^-1 b`` by a Cholesky factorisation in the arrays' own dtype (longdouble included)"""
    R = H.shape[0]
    Lm = np.array(H)
    for j in range(R):
        Lm[j, j] = np.sqrt(Lm[j, j])
        Lm[j + 1:, j] /= Lm[j, j]
        Lm[j + 1:, j + 1:] -= np.outer(Lm[j + 1:, j], Lm[j + 1:, j])
    u = np.array(b)
    for j in range(R):
        u[j] /= Lm[j, j]
        u[j + 1:] -= Lm[j + 1:, j] * u[j]
    for j in range(R - 1, -1, -1):
        u[j] /= Lm[j, j]
        u[:j] -= Lm[j, :j] * u[j]
    return u


def objective_parts(loss, Z, c, y, lam, theta):
    """``(F, g, H)`` of one column at ``theta``, in the dtype of ``Z``"""
    ls, d1, d2 = loss_terms(loss, c + Z @ theta, y.astype(Z.dtype))
    F = ls.sum() + (lam * theta * theta).sum() / 2
    return F, Z.T @ d1 + lam * theta, (Z.T * d2[None]) @ Z + np.diag(lam)


def newton(loss, Z, c, y, lam, max_iter, tol):
    """The damped Newton iteration of ``foldin_solve_kernel`` on one column: from zero; Newton
    step by Cholesky; Armijo backtracking (two values of ``F`` compared up to the rounding bound
    of its sum); stops at ``max |g| <= tol max |g(0)|``, at ``max_iter`` or when the line search
    stalls.  Returns ``(theta, n_iter, converged, max |g|, F(0), F(theta))``."""
    dtype = Z.dtype
    R = Z.shape[1]
    theta = np.zeros(R, dtype=dtype)
    F, g, H = objective_parts(loss, Z, c, y, lam, theta)
    F0, gn = F, (np.abs(g).max() if R else dtype.type(0))
    g0, n_iter = gn, 0
    eps = np.finfo(np.double).eps
    while n_iter < max_iter and not gn <= tol * g0:
        if dtype == np.double:
            s = np.linalg.solve(H, -g)
        else:
            s = _cholesky_solve(H, -g)
        slope, slack = g @ s, (Z.shape[0] + R + 2) * eps * F
        t, accepted = dtype.type(1), False
        for _ in range(HALVINGS + 1):
            trial = theta + t * s
            Ft = objective_parts(loss, Z, c, y, lam, trial)[0]
            if Ft <= F + ARMIJO * t * slope + slack:
                accepted = True
                break
            t = t / 2
        if not accepted:
            break
        theta, n_iter = trial, n_iter + 1
        F, g, H = objective_parts(loss, Z, c, y, lam, theta)
        gn = np.abs(g).max()
    return theta, n_iter, bool(gn <= tol * g0), gn, F0, F


def restate_fold_in(est, X, y, columns, alpha=None, beta=None, max_iter=50, tol=1e-8, wide=False,
                    n_threads=1):
    """Test aid, NumPy only, never touches the device: the design ``(Z, c)`` of every target
    column by the recurrence over each row's other entries, then the Newton iteration with the
    same rule.  ``wide``: in ``np.longdouble``.  Returns a ``FoldInResult`` that also holds
    ``theta`` (m, R), per column ``rows``, ``Z`` and ``c`` (lists), ``lam`` (R) the ridge
    strengths and ``problem`` the checked arguments.  ``n_threads``: design chunks and columns
    go side by side on that many host threads."""
    dtype = np.longdouble if wide else np.double
    pr = _problem(est, X, y, columns, alpha, beta, max_iter, tol, dtype)
    design = restate_design(pr, dtype, n_threads)
    lam = np.full(pr.R, pr.beta, dtype=dtype)
    if pr.lin:
        lam[0] = pr.alpha

    def solve(q):
        rows, Z, c = design[q]
        return newton(pr.loss, Z, c, pr.y[rows].astype(dtype), lam, pr.max_iter, pr.tol)

    sol = _map(solve, range(pr.cols.size), n_threads)
    theta = np.array([s[0] for s in sol], dtype=dtype).reshape(pr.cols.size, pr.R)
    return _result(est, pr, theta, [d[0].size for d in design], [s[1] for s in sol],
                   [s[2] for s in sol], [s[3] for s in sol], [s[4] for s in sol],
                   [s[5] for s in sol], rows=[d[0] for d in design],
                   Z=[d[1] for d in design], c=[d[2] for d in design], lam=lam, problem=pr)
