"""Pairwise ranking fit on the device: minibatch psgd over triples.

A training example is a triple ``(b, c+, c-)``: context row ``b`` of ``X`` prefers candidate
``c+`` of ``Z`` to candidate ``c-``.  With the margin

    m = f(x_b + z_c+) - f(x_b + z_c-)

the loss of a triple is ``loss(m, +1)`` -- ``'logistic'`` is BPR, ``'squared_hinge'`` and
``'squared'`` come with it -- and the penalties ``alpha/2 |w|^2 + beta/2 |P|^2 + gamma Omega(P)``,
the step sizes and the prox are exactly those of ``solver='psgd'``.  ``X`` and ``Z`` use the
vocabulary of ``ranking.py``: one feature space, disjoint column sets.  The stacked matrix
``[X; Z]`` goes to the device once per fit and a triple is three row indices into it
(``spfm_psgd_pairs_epoch``, ``include/spfm.h``): 12 bytes per triple, no materialised row
``x_b + z_c``, nothing to rebuild when the negatives are drawn again.

``sample_triples`` draws the negatives with NumPy (``sampler='host'``); ``sampler='uniform'`` and
``'dynamic'`` draw them on the device (``draw_u64`` / ``restate_sample``
restate that in NumPy).  ``restate_margins`` / ``restate_pair_gradient`` /
``restate_pairwise_epoch`` are plain NumPy restatements, test aids that never touch the device.
``objective='list'`` and ``'softmax'`` make a positive with its ``n_negatives`` negatives ONE
training item (``restate_list_scores`` / ``restate_list_gradient`` /
``restate_list_epoch`` restate it).
``sampler='warp'``, ``proposal=`` and ``sample_weight=`` are DESIGN.md section 19c: a weight per
triple, a weighted integer draw (``quantise_proposal`` / ``proposal_cum``) and the rank-weighted
sampler (``restate_warp``).
There is no CPU path of the fit: without the library or a GPU it raises.
"""
import numpy as np
import scipy.sparse as sp
from sklearn.utils import check_random_state
from sklearn.utils.validation import NotFittedError

from . import _capi
from .loss import CLASSIFICATION_LOSSES
from .ranking import _canonical, _check_disjoint, _pattern, _prepare, _widen
from .sparse_factorization_machines import MAX_DEGREE, _BaseSparseFactorizationMachine
from .monitor import callback_needs_params

PSGD_REGULARIZERS = ("l1", "l21", "squaredl12", "squaredl21")


# ------------------------------------------------------------------ negative sampling
def sample_triples(interactions, n_negatives=1, random_state=None, exclude=None):
    """``(m, 3)`` int32 triples ``(b, c+, c-)``: for every stored ``(b, c+)`` of the sparse
    ``(B, C)`` matrix ``interactions`` (pattern only), ``n_negatives`` candidates drawn uniformly
    from those stored neither in row ``b`` of ``interactions`` nor in row ``b`` of ``exclude``;
    ``m = nnz * n_negatives``, positives in canonical CSR order, the draws of one positive side by
    side.  Vectorised rejection: all draws at once, only the hits are drawn again.  Reproducible
    for a given seed.  ``ValueError`` for a row with a positive and no admissible candidate, and
    for ``m >= 2**31``."""
    if int(n_negatives) != n_negatives or n_negatives < 1:
        raise ValueError("n_negatives must be an integer >= 1, got %r" % (n_negatives,))
    n_negatives = int(n_negatives)
    if not sp.issparse(interactions):
        interactions = sp.csr_matrix(np.asarray(interactions))
    B, C = interactions.shape
    I = _pattern(interactions, B, C, "interactions")
    F = I
    if exclude is not None:
        F = (I + _pattern(exclude, B, C, "exclude")).tocsr()
        F.sort_indices()
    m = int(I.nnz) * n_negatives
    if m >= 2 ** 31:
        raise ValueError("%d triples: the triple list is limited to 2**31 - 1 rows" % m)
    full = (np.diff(F.indptr) >= C) & (np.diff(I.indptr) > 0)
    if full.any():
        raise ValueError("row %d stores every candidate (interactions and exclude together): no "
                         "negative can be drawn for it" % int(np.argmax(full)))
    rng = check_random_state(random_state)
    b = np.repeat(np.repeat(np.arange(B, dtype=np.int64), np.diff(I.indptr)), n_negatives)
    cp = np.repeat(I.indices.astype(np.int64), n_negatives)
    # (row, candidate) keys of the forbidden pairs, ascending: F is row-major with sorted indices
    keys = np.repeat(np.arange(B, dtype=np.int64), np.diff(F.indptr)) * C + F.indices
    cm = rng.randint(0, C, size=m).astype(np.int64)
    todo = np.arange(m)
    while todo.size:
        q = b[todo] * C + cm[todo]
        pos = np.searchsorted(keys, q)
        hit = (pos < keys.size) & (keys[np.minimum(pos, keys.size - 1)] == q)
        todo = todo[hit]
        if todo.size:
            cm[todo] = rng.randint(0, C, size=todo.size)
    return np.stack([b, cp, cm], axis=1).astype(np.int32)


def epoch_triples(rng, n_epochs, interactions=None, triples=None, n_negatives=1, resample=True,
                  shuffle=False, exclude=None, weights=None):
    """The triple list of every epoch of ``SparseFactorizationMachineRanker.fit``, in the order
    the device visits it, as the fit draws it from ``rng`` (a ``RandomState``): negatives are
    drawn before the first epoch and, with ``resample``, before every later one; with ``shuffle``
    the list is then permuted.  A generator of ``(m, 3)`` int32 arrays in context / candidate
    numbering.  ``weights`` (one per positive with ``interactions``, one per triple with
    ``triples``): ``(triples, weights per triple)`` pairs are generated instead, permuted
    together; the draws from ``rng`` do not change."""
    cur = None if triples is None else np.asarray(triples, dtype=np.int32)
    wcur = None
    if weights is not None:
        wcur = np.asarray(weights, dtype=np.double)
        if interactions is not None:
            wcur = np.repeat(wcur, int(n_negatives))
    for ep in range(n_epochs):
        if interactions is not None and (cur is None or resample):
            cur = sample_triples(interactions, n_negatives, rng, exclude)
        out, wout = cur, wcur
        if shuffle:
            perm = rng.permutation(cur.shape[0])
            out = cur[perm]
            wout = None if wcur is None else wcur[perm]
        yield out if wcur is None else (out, wout)


def check_triples(triples, B, C):
    """``(m, 3)`` int32 triples ``(b, c+, c-)`` in context / candidate numbering, checked against
    ``B`` contexts and ``C`` candidates; ``ValueError`` for a wrong shape, an index out of range,
    ``c+ == c-`` and ``m >= 2**31``.  Needs no device."""
    t = np.asarray(triples)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triples must have shape (m, 3), got %r" % (t.shape,))
    if t.shape[0] >= 2 ** 31:
        raise ValueError("%d triples: the triple list is limited to 2**31 - 1 rows" % t.shape[0])
    if t.size and not np.issubdtype(t.dtype, np.integer):
        if not np.all(t == np.floor(t)):
            raise ValueError("triples must hold integers")
    t = t.astype(np.int64)
    if t.size:
        if t[:, 0].min() < 0 or t[:, 0].max() >= B:
            raise ValueError("triples: context index out of range [0, %d)" % B)
        if t[:, 1:].min() < 0 or t[:, 1:].max() >= C:
            raise ValueError("triples: candidate index out of range [0, %d)" % C)
        same = np.flatnonzero(t[:, 1] == t[:, 2])
        if same.size:
            raise ValueError("triple %d has c+ == c- (candidate %d)"
                             % (int(same[0]), int(t[same[0], 1])))
    return np.ascontiguousarray(t, dtype=np.int32)


SAMPLERS = ("host", "uniform", "dynamic", "warp")
_MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    """the splitmix64 finaliser on uint64 arrays (arithmetic modulo 2**64)"""
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_u64(seed, epoch, r, t):
    """Test aid, NumPy only: draw ``t`` of output triple ``r`` in ``(seed, epoch)`` as the device
    sampler forms it (``sample_key`` / ``sample_draw``): stateless, integer
    arithmetic modulo 2**64, broadcasting over ``uint64`` arrays.

        a   = mix((seed << 32) ^ (epoch & 0xFFFFFFFF))
        key = mix(a ^ (r * 0x9E3779B97F4A7C15))
        u   = mix(key + (t + 1) * 0x9E3779B97F4A7C15)        mix: the splitmix64 finaliser

    The candidate of a draw is ``((u >> 32) * C) >> 32`` (``draw_candidates``)."""
    g = np.uint64(0x9E3779B97F4A7C15)
    seed, epoch, r, t = (np.asarray(v).astype(np.uint64) for v in (seed, epoch, r, t))
    with np.errstate(over="ignore"):
        a = _mix64((seed << np.uint64(32)) ^ (epoch & np.uint64(0xFFFFFFFF)))
        key = _mix64(a ^ (r * g))
        return _mix64(key + (t + np.uint64(1)) * g)


def draw_candidates(u, C, cum=None):
    """``((u >> 32) * C) >> 32`` on uint64 arrays: a candidate in ``[0, C)``; no floating point,
    no modulo.  With a proposal table ``cum`` (``proposal_cum``; ``W = cum[-1]``): the smallest
    ``c`` with ``cum[c] > ((u >> 32) * W) >> 32`` -- the same multiply-shift, then a search."""
    hi = np.asarray(u, dtype=np.uint64) >> np.uint64(32)
    if cum is None:
        return ((hi * np.uint64(C)) >> np.uint64(32)).astype(np.int64)
    cum = np.asarray(cum, dtype=np.uint64)
    if cum.shape != (C,):
        raise ValueError("cum must have shape (%d,), got %r" % (C, cum.shape))
    x = (hi * cum[-1]) >> np.uint64(32)
    return np.searchsorted(cum, x, side="right").astype(np.int64)


def quantise_proposal(weights, C=None):
    """Integer weights of a proposal distribution over the candidates, as the fit hands them to
    the device: ``q_c = max(floor(w_c / sum(w) * 2**31), 1 if w_c > 0 else 0)`` (int64).  A
    positive weight never becomes 0, a zero weight stays 0, and the total is at most
    ``2**31 + C < 2**32`` for every admissible ``C``.  ``ValueError`` for a negative or non-finite
    weight, a vector that is not ``(C,)``, and an all-zero vector."""
    w = np.asarray(weights, dtype=np.double)
    if w.ndim != 1 or (C is not None and w.shape[0] != C):
        raise ValueError("proposal must hold one weight per candidate%s, got shape %r"
                         % ("" if C is None else " (%d)" % C, w.shape))
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("proposal: the weights must be finite and >= 0")
    if not (w > 0).any():
        raise ValueError("proposal: every weight is zero")
    q = np.floor(w / w.sum() * float(2 ** 31)).astype(np.int64)
    return np.maximum(q, (w > 0).astype(np.int64))


def proposal_cum(q):
    """the inclusive cumulative sums of the integer weights ``q`` as uint32
    (``spfm_psgd_pairs_set_proposal``)"""
    cum = np.cumsum(np.asarray(q, dtype=np.int64))
    if (np.asarray(q) < 0).any() or cum[-1] < 1 or cum[-1] >= 2 ** 32:
        raise ValueError("proposal: the integer weights must be >= 0 with a total in [1, 2**32)")
    return cum.astype(np.uint32)


def popularity_weights(interactions, power=0.75):
    """``(stored entries of the candidate's column of interactions + 1) ** power``"""
    I = sp.csr_matrix(interactions)
    return (np.bincount(I.indices, minlength=I.shape[1]) + 1.0) ** float(power)


def _forbidden(interactions, exclude, B, C):
    """(I, F): the canonical patterns of the positives and of ``interactions`` + ``exclude``"""
    I = _pattern(interactions, B, C, "interactions")
    F = I
    if exclude is not None:
        F = (I + _pattern(exclude, B, C, "exclude")).tocsr()
        F.sort_indices()
    full = (np.diff(F.indptr) >= C) & (np.diff(I.indptr) > 0)
    if full.any():
        raise ValueError("row %d stores every candidate (interactions and exclude together): no "
                         "negative can be drawn for it" % int(np.argmax(full)))
    return I, F


def _admitted_sets(I, F, n_negatives, n_candidates, max_draws, seed, epoch, cum=None):
    """per output triple r: (b, c+, the admitted candidates in the order of their draws); the
    fallback candidate alone where no draw with t < max_draws is admitted"""
    B, C = I.shape
    rows = np.repeat(np.arange(B), np.diff(I.indptr))
    t = np.arange(max_draws, dtype=np.uint64)
    out = []
    for r in range(I.nnz * n_negatives):
        q = r // n_negatives
        b = int(rows[q])
        forb = F.indices[F.indptr[b]:F.indptr[b + 1]]
        cand = draw_candidates(draw_u64(seed, epoch, r, t), C, cum)
        adm = cand[~np.isin(cand, forb)][:n_candidates]
        walked = adm.size == 0
        if walked:  # upwards, cyclically, from the last drawn candidate
            c = int(cand[-1])
            for _ in range(C):
                c = 0 if c + 1 == C else c + 1
                if c not in forb:
                    break
            adm = np.array([c], dtype=np.int64)
        out.append((b, int(I.indices[q]), adm, walked))
    return out


def restate_sample(P, w, lams, X, Z, interactions, degree, n_negatives, n_candidates, max_draws,
                   seed, epoch, exclude=None, order=None, wide=False, details=False, cum=None):
    """Test aid, NumPy only: what ``spfm_psgd_pairs_sample`` leaves on the device.  For output
    triple ``r = q * n_negatives + i`` (positive ``q`` of ``interactions`` in canonical CSR order)
    the first ``n_candidates`` admitted draws among ``t < max_draws`` (admitted: the candidate is
    stored neither in row ``b`` of ``interactions`` nor of ``exclude``; none admitted: the first
    admissible candidate upwards, cyclically, from the last drawn one), scored by dense evaluation
    of ``s(b, c) = sum_o sum_s lams_s a_s^{degree-o}(x_b + z_c) + <w, z_c>``; the negative is the
    one with the largest score, ties to the earliest draw.  Returns ``(triples, scores, gap)`` by
    slot (``order[r]``, or ``r``): ``(m, 3)`` int32 in context / candidate numbering, the chosen
    scores (zeros for ``n_candidates == 1``, which scores nothing) and the distance between the
    best score and the best score of a *different* candidate of the set (``inf`` without one).
    ``details``: a fourth item, per ``r`` (not slot) the pair (admitted candidates, their
    scores).  ``cum``: the proposal table of the draws (``draw_candidates``)."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = P[None] if P.ndim == 2 else P
    B, C = X.shape[0], Z.shape[0]
    if not sp.issparse(interactions):
        interactions = sp.csr_matrix(np.asarray(interactions))
    I, F = _forbidden(interactions, exclude, B, C)
    sets = _admitted_sets(I, F, int(n_negatives), int(n_candidates), int(max_draws), seed, epoch,
                          cum)
    m = len(sets)
    row_scores = _row_scorer(P, w, lams, X, Z, degree, dtype)
    slots = np.arange(m) if order is None else np.asarray(order, dtype=np.int64)
    triples = np.empty((m, 3), dtype=np.int32)
    scores = np.zeros(m, dtype=dtype)
    gap = np.full(m, np.inf)
    det = []
    for r, (b, cp, adm, _) in enumerate(sets):
        sc = row_scores(b)[adm]
        best = int(np.argmax(sc))  # the first maximum: the earliest admitted draw
        other = sc[adm != adm[best]]
        if other.size:
            gap[slots[r]] = float(sc[best] - other.max())
        triples[slots[r]] = (b, cp, adm[best])
        if n_candidates > 1:
            scores[slots[r]] = sc[best]
        det.append((adm, sc))
    if details:
        return triples, scores, gap, det
    return triples, scores, gap


def _row_scorer(P, w, lams, X, Z, degree, dtype):
    """b -> the scores s(b, .) of every candidate by dense evaluation, cached per context"""
    Xd, Zd = _dense_sides(X, Z, dtype)
    lin = Zd @ w
    cache = {}

    def row_scores(b):
        if b not in cache:
            cache[b] = _rows_output(P, lams, Xd[b][None, :] + Zd, degree)[0] + lin
        return cache[b]

    return row_scores


def restate_warp(P, w, lams, X, Z, interactions, degree, n_negatives, max_trials, max_draws,
                 margin, seed, epoch, exclude=None, order=None, wide=False, cum=None,
                 positive_weights=None, details=False):
    """Test aid, NumPy only: what ``spfm_psgd_pairs_sample_warp`` leaves on the device (DESIGN.md
    section 19c).  The draws, the admission, the score and the slots are ``restate_sample``'s.
    For output triple ``r`` of positive ``q = (b, c+)`` the admitted draws with ``t < max_draws``
    are tried in the order of ``t``, at most ``max_trials`` of them; the first ``a_N`` with
    ``s(b, a_N) > s(b, c+) - margin`` is the negative, ``trials = N`` and ``weight = posw_q *
    log(max(1, A_b // N))`` with ``A_b = C - |forbidden(b)|``.  No violator: the highest-scored of
    those tried (ties to the earliest), ``trials = 0``, ``weight = 0``; no draw admitted: the
    fallback walk's candidate, ``trials = 0``, ``weight = 0``.  Returns ``(triples, scores,
    weights, trials, near)`` by slot; ``near`` is the smallest ``|s - (s+ - margin)|`` over the
    candidates that were tried (``inf`` for the fallback).  ``details``: a sixth item, per ``r``
    (not slot) ``(tried candidates, their scores, s+ - margin)``."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = P[None] if P.ndim == 2 else P
    B, C = X.shape[0], Z.shape[0]
    if not sp.issparse(interactions):
        interactions = sp.csr_matrix(np.asarray(interactions))
    I, F = _forbidden(interactions, exclude, B, C)
    if max_trials < 1 or max_trials > max_draws:
        raise ValueError("1 <= max_trials <= max_draws is required")
    sets = _admitted_sets(I, F, int(n_negatives), int(max_trials), int(max_draws), seed, epoch,
                          cum)
    m = len(sets)
    posw = (np.ones(I.nnz) if positive_weights is None
            else np.asarray(positive_weights, dtype=np.double))
    if posw.shape != (I.nnz,):
        raise ValueError("positive_weights must have shape (%d,)" % I.nnz)
    row_scores = _row_scorer(P, w, lams, X, Z, degree, dtype)
    free = C - np.diff(F.indptr)
    slots = np.arange(m) if order is None else np.asarray(order, dtype=np.int64)
    triples = np.empty((m, 3), dtype=np.int32)
    scores = np.zeros(m, dtype=dtype)
    weights = np.zeros(m)
    trials = np.zeros(m, dtype=np.int32)
    near = np.full(m, np.inf)
    det = []
    for r, (b, cp, adm, walked) in enumerate(sets):
        s_all = row_scores(b)
        thr = s_all[cp] - dtype(margin)
        sc = s_all[adm]
        viol = np.flatnonzero(sc > thr)
        if walked:
            pick, n_tried = 0, 0
        elif viol.size:
            pick = int(viol[0])
            n_tried = pick + 1
            trials[slots[r]] = n_tried
            rank = max(1, int(free[b]) // n_tried)
            weights[slots[r]] = posw[r // int(n_negatives)] * np.log(float(rank))
        else:
            pick, n_tried = int(np.argmax(sc)), adm.size
        if n_tried:
            near[slots[r]] = float(np.abs(sc[:n_tried] - thr).min())
        triples[slots[r]] = (b, cp, adm[pick])
        scores[slots[r]] = sc[pick]
        det.append((adm[:n_tried], sc[:n_tried], thr))
    if details:
        return triples, scores, weights, trials, near, det
    return triples, scores, weights, trials, near


def _prepare_pairs(est, X, Z):
    """Canonical, checked, widened (X, Z) of one width, for an estimator that need not be fitted;
    every argument error is raised here, before a handle exists."""
    X = _canonical(X)
    Z = _canonical(Z)
    if X.shape[1] != Z.shape[1]:
        raise ValueError("X has %d features, Z has %d" % (X.shape[1], Z.shape[1]))
    if X.shape[0] < 1 or Z.shape[0] < 2:
        raise ValueError("a pairwise fit needs a context row and two candidate rows")
    _check_disjoint(X, Z)
    return _widen(est, X, Z)


def _check_weights(weights, count, what):
    """``None``, or ``count`` finite weights ``>= 0`` as float64 (one per ``what``)"""
    if weights is None:
        return None
    wt = np.asarray(weights, dtype=np.double)
    if wt.shape != (count,):
        raise ValueError("sample_weight must hold one value per %s (%d), got shape %r"
                         % (what, count, wt.shape))
    if not np.isfinite(wt).all() or (wt < 0).any():
        raise ValueError("sample_weight: the weights must be finite and >= 0")
    return np.ascontiguousarray(wt)


# ------------------------------------------------------------------ NumPy restatement (test aid)
def _loss_pos(loss, m):
    """loss(m, +1) and its derivative, as ``loss_dev`` / ``dloss_dev`` compute them"""
    one = m.dtype.type(1)
    if loss == "squared":
        return (m - one) * (m - one) / 2, m - one
    if loss == "squared_hinge":
        z = one - m
        return np.where(z > 0, z * z, 0), np.where(z > 0, -2 * z, 0)
    if loss == "logistic":
        mc = np.clip(m, -18, 18)
        val = np.where(m > 18, np.exp(-m), np.where(m < -18, -m, np.log(1 + np.exp(-mc))))
        der = np.where(m > 18, -np.exp(-m), np.where(m < -18, -one, -one / (np.exp(mc) + 1)))
        return val, der
    raise ValueError("Loss function %r is not supported." % (loss,))


def _dense_sides(X, Z, dtype):
    Xd = np.asarray(sp.csr_matrix(X).todense(), dtype=dtype)
    Zd = np.asarray(sp.csr_matrix(Z).todense(), dtype=dtype)
    return Xd, Zd


def _anova_rows(Po, V, deg):
    """a[t] (t = 0..deg), each (n, k): the ANOVA DP of the rows V (n, d) with P_o (k, d)"""
    n, k = V.shape[0], Po.shape[0]
    a = [np.ones((n, k), dtype=V.dtype)] + [np.zeros((n, k), dtype=V.dtype) for _ in range(deg)]
    for j in np.flatnonzero(np.any(V != 0, axis=0)):
        px = V[:, j, None] * Po[None, :, j]
        for t in range(deg, 0, -1):
            a[t] = a[t] + a[t - 1] * px
    return a


def _rows_output(P, lams, V, degree):
    """sum over the orders o (degree ``degree - o``) of sum_s lams_s a^deg_s(row), and the DP
    arrays per order"""
    out = np.zeros(V.shape[0], dtype=V.dtype)
    dps = []
    for o in range(P.shape[0]):
        a = _anova_rows(P[o], V, degree - o)
        dps.append(a)
        out = out + a[degree - o] @ lams
    return out, dps


def _as(dtype, *arrays):
    return tuple(np.asarray(a, dtype=dtype) for a in arrays)


def restate_margins(P, w, lams, X, Z, triples, degree, wide=False):
    """Test aid, NumPy only: the margins ``f(x_b + z_c+) - f(x_b + z_c-)`` of the triples
    ``(b, c+, c-)`` (context / candidate numbering) by evaluating the ANOVA recurrence on both
    dense summed rows; every order ``o`` of ``P`` (n_orders, k, d) enters with degree
    ``degree - o``, as in the minibatch solver, and ``w`` as it stands.  float64, or
    ``np.longdouble`` with ``wide``."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = P[None] if P.ndim == 2 else P
    Xd, Zd = _dense_sides(X, Z, dtype)
    t = np.asarray(triples, dtype=np.int64)
    fp, _ = _rows_output(P, lams, Xd[t[:, 0]] + Zd[t[:, 1]], degree)
    fm, _ = _rows_output(P, lams, Xd[t[:, 0]] + Zd[t[:, 2]], degree)
    return (fp - fm) + (Zd[t[:, 1]] - Zd[t[:, 2]]) @ w


def restate_pair_gradient(P, w, lams, X, Z, triples, degree, loss, wide=False, weights=None):
    """Test aid, NumPy only: ``(losses (m,), grad_P (n_orders, k, d), grad_w (d,))`` of the
    summed loss of the triples at ``(P, w)`` -- the sums one minibatch scatters.  ``grad_w`` is
    formed from ``z_c+ - z_c-`` alone: the context's term cancels and its columns are exactly
    zero.  ``weights`` (m,): triple ``q`` enters with ``weights[q]`` times its loss (the returned
    losses are weighted too)."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = P[None] if P.ndim == 2 else P
    Xd, Zd = _dense_sides(X, Z, dtype)
    t = np.asarray(triples, dtype=np.int64)
    Vp, Vm = Xd[t[:, 0]] + Zd[t[:, 1]], Xd[t[:, 0]] + Zd[t[:, 2]]
    fp, dpp = _rows_output(P, lams, Vp, degree)
    fm, dpm = _rows_output(P, lams, Vm, degree)
    dz = Zd[t[:, 1]] - Zd[t[:, 2]]
    val, dL = _loss_pos(loss, (fp - fm) + dz @ w)
    if weights is not None:
        wt = np.asarray(weights, dtype=dtype)
        val, dL = wt * val, wt * dL
    gP = np.zeros_like(P)
    for o in range(P.shape[0]):
        deg = degree - o
        for V, dps, sign in ((Vp, dpp[o], 1), (Vm, dpm[o], -1)):
            # _grad_anova: d a^deg / d p_sj by the recurrence dprev <- x (a[t] - p dprev)
            x = V[:, None, :]
            dprev = np.broadcast_to(x, (V.shape[0], P.shape[1], V.shape[1]))
            for tt in range(1, deg):
                dprev = x * (dps[tt][:, :, None] - P[o][None] * dprev)
            gP[o] += sign * np.einsum("r,s,rsj->sj", dL, lams, dprev)
    return val, gP, dL @ dz


def _psgd_eta(learning_rate, eta0, alpha, beta, power_t, it):
    """optimizer/psgd.py:9-22 (``spfm_engine::psgd_eta``)"""
    lr = _capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str) else learning_rate
    if lr == 0:
        return eta0, eta0
    if lr == 1:
        e = eta0 * float(it)
        return eta0 / (1.0 + e * beta) ** power_t, eta0 / (1.0 + e * alpha) ** power_t
    if lr == 2:
        return 1.0 / (beta * float(it)), 1.0 / (alpha * float(it))
    e = eta0 / float(it) ** power_t
    return e, e


def _soft(v, thr):
    return np.sign(v) * np.maximum(np.abs(v) - thr, 0)


def _prox_squaredl12(p, c):
    """prox of c (sum_i |p_i|)^2 by the monotone Michelot fixed point the device iterates:
    G <- {i : |p_i| >= tau(G)}, tau(G) = 2 c S_G / (1 + 2 c |G|), from G = all"""
    a = np.abs(p)
    cond, theta = a.dtype.type(0), -1
    while True:
        G = a >= cond
        S, th = a[G].sum(), int(G.sum())
        den = 1 + 2 * c * th
        cond = 2 * c * S / den
        if th == theta:
            return _soft(p, 2 * c * (S / den))
        theta = th


def _prox(regularizer, Po, c):
    """regularizer.prox on one order's block P_o (k, d), features along the second axis"""
    if regularizer == "l1":
        return _soft(Po, c)
    if regularizer == "l21":
        nr = np.sqrt((np.abs(Po) ** 2).sum(axis=0))
        nr = np.where(nr <= c, np.inf, nr)
        return Po * (1 - c / nr)
    if regularizer == "squaredl12":
        return np.stack([_prox_squaredl12(Po[s], c) for s in range(Po.shape[0])])
    if regularizer == "squaredl21":
        nr = np.sqrt((np.abs(Po) ** 2).sum(axis=0))
        unit = Po / np.where(nr > 0, nr, 1)
        return unit * _prox_squaredl12(nr, c)
    raise ValueError("regularizer %r cannot be used with a pairwise fit" % (regularizer,))


def _adaptive_step(P, w, gP, gw, B, eta_P, eta_w, alpha, beta, gamma, regularizer, fit_linear,
                   G0, acc):
    """one minibatch of the per-feature AdaGrad rule from the summed
    gradients; ``acc = (A_P (n_orders, d), A_w (d,))`` is updated in place.  -> (P, w)"""
    if regularizer not in ("l1", "l21"):
        raise ValueError("adaptive steps cannot be combined with regularizer %r: its prox couples "
                         "features that carry different steps" % (regularizer,))
    dtype = P.dtype.type
    A_P, A_w = acc
    if fit_linear:
        gb = gw / B
        A_w += gb ** 2
        ew = eta_w / np.sqrt(dtype(G0) + A_w)
        w = (w - ew * gb) / (1 + ew * alpha)
    gb = gP / B
    A_P += (gb ** 2).sum(axis=1)
    e = (eta_P / np.sqrt(dtype(G0) + A_P))[:, None, :]  # one step per (order, feature)
    P = (P - e * gb) / (1 + e * beta)
    c = gamma * e / (1 + e * beta)
    if regularizer == "l1":
        return _soft(P, c), w
    nr = np.sqrt((np.abs(P) ** 2).sum(axis=1, keepdims=True))
    nr = np.where(nr <= c, np.inf, nr)
    return P * (1 - c / nr), w


def _adaptive_state(adaptive, acc, P, dtype):
    """(G0 or None, (A_P, A_w) copies in ``dtype``) of the restatements' ``adaptive`` / ``acc``"""
    if adaptive is None:
        return None, acc
    if adaptive is True or adaptive == "adagrad":
        G0 = 1.0
    else:
        G0 = float(adaptive)
    if not (G0 > 0 and np.isfinite(G0)):
        raise ValueError("adaptive: the initial accumulator must be positive and finite")
    if acc is None:
        return G0, (np.zeros((P.shape[0], P.shape[2]), dtype=dtype),
                    np.zeros(P.shape[2], dtype=dtype))
    return G0, (np.array(acc[0], dtype=dtype), np.array(acc[1], dtype=dtype))


def restate_pairwise_epoch(P, w, lams, X, Z, triples, degree, loss="logistic", regularizer="l1",
                           alpha=1.0, beta=1.0, gamma=1.0, eta0=1.0, learning_rate="optimal",
                           power_t=1.0, batch_size=1, fit_linear=True, it=1, wide=False,
                           weights=None, adaptive=None, acc=None):
    """Test aid, NumPy only: one epoch of the pairwise fit over ``triples`` (context / candidate
    numbering, visited in the order given) from ``P`` (n_orders, k, d) and ``w``.  Minibatch
    ``bi`` covers the triples ``[bi * batch_size, ...)``, the last one may be shorter; per batch
    the gradient sums, the step ``eta / B`` with ``psgd_eta`` at ``it``, the shrink and the prox of
    the minibatch solver.  ``weights`` (m,): one per triple, visited with it; the step stays
    ``eta / B`` with ``B`` the triple count and ``sum_loss`` is the sum of weight times loss.
    Returns ``(P, w, sum_loss, it)`` (new arrays).

    ``adaptive``: ``None`` is the above; ``True`` / ``'adagrad'`` (G0 = 1)
    or a positive G0 steps every feature with ``eta / sqrt(G0 + A)`` -- ``learning_rate`` gives
    the base rate ``eta``, ``acc = (A_P (n_orders, d), A_w (d,))`` the accumulators to start from
    (``None``: zeros) -- and the return value is ``(P, w, sum_loss, it, (A_P, A_w))``."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = (P[None] if P.ndim == 2 else P).copy()
    w = w.copy()
    t = np.asarray(triples, dtype=np.int64)
    sum_loss = dtype(0)
    G0, acc = _adaptive_state(adaptive, acc, P, dtype)
    for pos in range(0, t.shape[0], int(batch_size)):
        tb = t[pos:pos + int(batch_size)]
        wb = None if weights is None else np.asarray(weights)[pos:pos + int(batch_size)]
        val, gP, gw = restate_pair_gradient(P, w, lams, X, Z, tb, degree, loss, wide, wb)
        sum_loss += val.sum()
        eta_P, eta_w = _psgd_eta(learning_rate, eta0, alpha, beta, power_t, it)
        if G0 is not None:
            P, w = _adaptive_step(P, w, gP, gw, tb.shape[0], eta_P, eta_w, alpha, beta, gamma,
                                  regularizer, fit_linear, G0, acc)
            it += 1
            continue
        if fit_linear:
            w = (w - gw * (eta_w / tb.shape[0])) / (1 + eta_w * alpha)
        P = (P - gP * (eta_P / tb.shape[0])) / (1 + eta_P * beta)
        strength = gamma * eta_P / (1 + eta_P * beta)
        P = np.stack([_prox(regularizer, P[o], dtype(strength)) for o in range(P.shape[0])])
        it += 1
    if G0 is not None:
        return P, w, sum_loss, it, acc
    return P, w, sum_loss, it


# ------------------------------------------------------------------ lists
OBJECTIVES = ("pairwise", "list", "softmax")


def check_lists(triples, n_negatives, objective="softmax"):
    """The list arguments of the fit, checked without a device: ``objective`` one of
    ``'list'``, ``'softmax'``; ``n_negatives`` an integer in ``[1, SPFM_LIST_MAX_NEG]``; and, when
    ``triples`` is given, ``(m, 3)`` rows grouped by list -- ``m`` a multiple of ``n_negatives``,
    rows ``q M .. q M + M - 1`` with one context and one ``c+``.  ``ValueError`` otherwise."""
    if objective not in OBJECTIVES[1:]:
        raise ValueError("objective %r is not a list objective. Choose from %s."
                         % (objective, list(OBJECTIVES[1:])))
    if int(n_negatives) != n_negatives or not 1 <= n_negatives <= _capi.LIST_MAX_NEG:
        raise ValueError("objective=%r: n_negatives must be an integer in [1, %d], got %r"
                         % (objective, _capi.LIST_MAX_NEG, n_negatives))
    if triples is None:
        return
    t = np.asarray(triples)
    M = int(n_negatives)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triples must have shape (m, 3), got %r" % (t.shape,))
    if t.shape[0] % M:
        raise ValueError("objective=%r: %d triples are not a multiple of n_negatives = %d"
                         % (objective, t.shape[0], M))
    head = np.repeat(t[::M, :2], M, axis=0)
    bad = np.flatnonzero((t[:, :2] != head).any(axis=1))
    if bad.size:
        raise ValueError("objective=%r: triple %d differs from the first of its list in context "
                         "or c+: the triples must be grouped, n_negatives rows per positive"
                         % (objective, int(bad[0])))


def _list_candidates(triples, n_negatives):
    """(contexts (Q,), candidates (Q, M + 1)) of grouped triples; column 0 is the positive"""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, int(n_negatives), 3)
    return t[:, 0, 0], np.concatenate([t[:, :1, 1], t[:, :, 2]], axis=1)


def restate_list_scores(P, w, lams, X, Z, triples, n_negatives, degree, wide=False):
    """Test aid, NumPy only: the scores ``s_i = s(b, c_i)`` of every list of the grouped
    ``triples``, ``(Q, M + 1)`` with the positive in column 0 -- every order of ``P``, ``w`` as it
    stands, the context's linear term left out (``restate_sample``'s score)."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = P[None] if P.ndim == 2 else P
    Xd, Zd = _dense_sides(X, Z, dtype)
    b, cand = _list_candidates(triples, n_negatives)
    cols = [_rows_output(P, lams, Xd[b] + Zd[cand[:, i]], degree)[0] + Zd[cand[:, i]] @ w
            for i in range(cand.shape[1])]
    return np.stack(cols, axis=1)


def _list_coefs(s, objective, loss):
    """(loss per list (Q,), coef = dLoss/ds (Q, M + 1)) from the scores"""
    M = s.shape[1] - 1
    if objective == "softmax":
        mx = s.max(axis=1)
        ex = np.exp(s - mx[:, None])
        z = ex.sum(axis=1)
        coef = ex / z[:, None]
        coef[:, 0] -= 1
        return (mx - s[:, 0]) + np.log(z), coef
    if objective != "list":
        raise ValueError("objective %r is not a list objective" % (objective,))
    val, der = _loss_pos(loss, s[:, :1] - s[:, 1:])
    coef = np.empty_like(s)
    coef[:, 1:] = -der / M
    coef[:, 0] = -coef[:, 1:].sum(axis=1)
    return val.sum(axis=1) / M, coef


def restate_list_gradient(P, w, lams, X, Z, triples, n_negatives, degree, objective="softmax",
                          loss="logistic", wide=False):
    """Test aid, NumPy only: ``(losses (Q,), grad_P (n_orders, k, d), grad_w (d,))`` of the
    summed loss of the lists at ``(P, w)``.  ``'softmax'``: ``-s_0 + log sum_i exp(s_i)``;
    ``'list'``: ``(1/M) sum_{i>=1} loss(s_0 - s_i, +1)``.  The gradient is the plain sum over the
    ``M + 1`` candidates of ``coef_i`` times the gradient of ``s_i`` on the dense row
    ``x_b + z_{c_i}`` -- the device's combined DP array is NOT used here.  ``grad_w`` is formed
    from the ``z_{c_i}`` alone: the coefficients of a list sum to zero and the context's columns
    are exactly zero."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = P[None] if P.ndim == 2 else P
    Xd, Zd = _dense_sides(X, Z, dtype)
    b, cand = _list_candidates(triples, n_negatives)
    rows, dps, cols = [], [], []
    for i in range(cand.shape[1]):
        V = Xd[b] + Zd[cand[:, i]]
        f, dp = _rows_output(P, lams, V, degree)
        rows.append(V)
        dps.append(dp)
        cols.append(f + Zd[cand[:, i]] @ w)
    val, coef = _list_coefs(np.stack(cols, axis=1), objective, loss)
    gP = np.zeros_like(P)
    gw = np.zeros_like(w)
    for i, V in enumerate(rows):
        gw += coef[:, i] @ Zd[cand[:, i]]
        x = V[:, None, :]
        for o in range(P.shape[0]):
            dprev = np.broadcast_to(x, (V.shape[0], P.shape[1], V.shape[1]))
            for tt in range(1, degree - o):
                dprev = x * (dps[i][o][tt][:, :, None] - P[o][None] * dprev)
            gP[o] += np.einsum("r,s,rsj->sj", coef[:, i], lams, dprev)
    return val, gP, gw


def restate_list_epoch(P, w, lams, X, Z, triples, n_negatives, degree, objective="softmax",
                       loss="logistic", regularizer="l1", alpha=1.0, beta=1.0, gamma=1.0,
                       eta0=1.0, learning_rate="optimal", power_t=1.0, batch_size=1,
                       fit_linear=True, it=1, wide=False, adaptive=None, acc=None):
    """Test aid, NumPy only: one epoch of the list fit over the grouped ``triples`` (lists
    visited in the order given).  ``restate_pairwise_epoch`` with lists as items: minibatch ``bi``
    covers the lists ``[bi * batch_size, ...)``, the step is ``eta / B`` with ``B`` lists.
    Returns ``(P, w, sum_loss over the lists, it)`` (new arrays); with ``adaptive`` / ``acc`` as in
    ``restate_pairwise_epoch``, ``(P, w, sum_loss, it, (A_P, A_w))``."""
    dtype = np.longdouble if wide else np.double
    P, w, lams = _as(dtype, P, w, lams)
    P = (P[None] if P.ndim == 2 else P).copy()
    w = w.copy()
    M = int(n_negatives)
    t = np.asarray(triples, dtype=np.int64)
    sum_loss = dtype(0)
    G0, acc = _adaptive_state(adaptive, acc, P, dtype)
    for pos in range(0, t.shape[0] // M, int(batch_size)):
        tb = t[pos * M:(pos + int(batch_size)) * M]
        B = tb.shape[0] // M
        val, gP, gw = restate_list_gradient(P, w, lams, X, Z, tb, M, degree, objective, loss,
                                            wide)
        sum_loss += val.sum()
        eta_P, eta_w = _psgd_eta(learning_rate, eta0, alpha, beta, power_t, it)
        if G0 is not None:
            P, w = _adaptive_step(P, w, gP, gw, B, eta_P, eta_w, alpha, beta, gamma, regularizer,
                                  fit_linear, G0, acc)
            it += 1
            continue
        if fit_linear:
            w = (w - gw * (eta_w / B)) / (1 + eta_w * alpha)
        P = (P - gP * (eta_P / B)) / (1 + eta_P * beta)
        strength = gamma * eta_P / (1 + eta_P * beta)
        P = np.stack([_prox(regularizer, P[o], dtype(strength)) for o in range(P.shape[0])])
        it += 1
    if G0 is not None:
        return P, w, sum_loss, it, acc
    return P, w, sum_loss, it


def epoch_lists(rng, n_epochs, interactions=None, triples=None, n_negatives=1, resample=True,
                shuffle=False, exclude=None):
    """``epoch_triples`` for the list objectives: the grouped triples of every epoch, with
    ``shuffle`` the LISTS permuted (``rng.permutation(Q)``), never the rows within one."""
    M = int(n_negatives)
    cur = None if triples is None else np.asarray(triples, dtype=np.int32)
    for ep in range(n_epochs):
        if interactions is not None and (cur is None or resample):
            cur = sample_triples(interactions, M, rng, exclude)
        out = cur
        if shuffle:
            out = cur.reshape(-1, M, 3)[rng.permutation(cur.shape[0] // M)].reshape(-1, 3)
        yield out


# ------------------------------------------------------------------ the estimator
class SparseFactorizationMachineRanker(_BaseSparseFactorizationMachine):
    """Factorization machine trained for an order: minibatch psgd on the pairwise loss
    ``loss(f(x_b + z_c+) - f(x_b + z_c-), +1)`` over triples.  The constructor takes the keywords
    of the classifier (``loss='logistic'``: BPR); ``solver`` must be ``'psgd'``, the regularizer
    one of ``'l1'``, ``'l21'``, ``'squaredl12'``, ``'squaredl21'``, and ``distributed`` False.
    The fitted object has ``P_``, ``w_``, ``lams_`` like every estimator here: ``ranker``,
    ``rank_metrics``, ``fold_in``, the explain calls and the interaction views work on it."""

    _LOSSES = CLASSIFICATION_LOSSES

    def __init__(
        self,
        degree=2,
        loss="logistic",
        n_components=2,
        solver="psgd",
        regularizer="squaredl12",
        alpha=1,
        beta=1,
        gamma=1,
        mean=False,
        tol=1e-6,
        fit_lower="explicit",
        fit_linear=True,
        warm_start=False,
        init_lambdas="ones",
        max_iter=100,
        shuffle=False,
        batch_size="auto",
        eta0=1.0,
        learning_rate="optimal",
        power_t=1.0,
        n_iter_no_change=5,
        verbose=False,
        callback=None,
        n_calls=10,
        random_state=None,
        schedule="exact",
        precision="f32",
        device=None,
        distributed=False,
    ):
        super(SparseFactorizationMachineRanker, self).__init__(
            degree, loss, n_components, solver, regularizer, alpha, beta, gamma, mean, tol,
            fit_lower, fit_linear, warm_start, init_lambdas, max_iter, shuffle, batch_size, eta0,
            learning_rate, power_t, n_iter_no_change, verbose, callback, n_calls, random_state,
            schedule, precision, device, distributed,
        )

    def _check_config(self):
        if self.solver != "psgd":
            raise ValueError("Solver %s is not supported by the pairwise fit: it is minibatch "
                             "psgd over triples (solver='psgd')." % (self.solver,))
        if self.regularizer not in PSGD_REGULARIZERS:
            raise ValueError("regularizer %r cannot be used with the pairwise fit; choose from %s"
                             % (self.regularizer, list(PSGD_REGULARIZERS)))
        if self.distributed:
            raise ValueError("the pairwise fit runs on one GPU (distributed=False).")
        self._get_loss(self.loss)
        self._check_adagrad(self.regularizer, False)
        if self._base_rate() not in _capi.LEARNING_RATE:
            raise ValueError("learning_rate %s is not supported. Choose from %s."
                             % (self.learning_rate, _capi.LEARNING_RATE))
        if self.degree > MAX_DEGREE:
            raise NotImplementedError("degree > %d is not supported by the HIP engine"
                                      % MAX_DEGREE)

    def fit(self, X, Z, interactions=None, triples=None, n_negatives=1, resample=True,
            sampler="host", n_candidates=8, exclude=None, objective="pairwise", margin=1.0,
            proposal=None, proposal_power=0.75, sample_weight=None):
        """Fit on contexts ``X`` (B, d) and candidates ``Z`` (C, d) with disjoint column sets.
        Exactly one of ``interactions`` -- a sparse (B, C) matrix whose stored entries are the
        positives; ``n_negatives`` negatives per positive are drawn, again before every epoch
        when ``resample`` -- and ``triples`` -- (m, 3) rows ``(b, c+, c-)`` in context /
        candidate numbering -- is given.  ``exclude`` (sparse (B, C), pattern only): candidates
        that are never drawn as negatives of a context, besides its positives.  ``sampler``:

        * ``'host'``: ``sample_triples`` (NumPy, uniform); an epoch uploads its 12 m bytes.
        * ``'uniform'``: the device draws them, uniformly.
        * ``'dynamic'``: the device draws ``n_candidates`` admissible candidates per triple and
          trains against the one the current parameters score highest (dynamic negative
          sampling; the choice is made once per epoch, at the epoch's first parameters).

        The device samplers take one seed from ``random_state`` after the parameter
        initialisation and use the epoch number as the stream's second key; with ``shuffle`` a
        permutation of the slots (4 m bytes) is uploaded per sampling; with ``resample=False``
        they sample once and every epoch visits that one list.  ``[X; Z]`` is uploaded once.
        Stopping rule, ``verbose`` lines, callbacks, ``it_``, ``n_iter_`` and ``warm_start`` as
        for ``solver='psgd'``, with the mean loss per triple.

        ``objective``: ``'pairwise'`` is the above.  ``'softmax'`` and
        ``'list'`` make a positive and its ``n_negatives`` (at most 63) negatives one training
        item: ``'softmax'`` is the sampled softmax ``-s_0 + log sum_i exp(s_i)``, ``'list'`` the
        mean of the ``n_negatives`` pairwise losses (the pairwise fit's arithmetic with
        ``batch_size`` counted in positives).  ``batch_size``, the shuffle and the mean loss of
        the stopping rule count lists; explicit ``triples`` must arrive grouped, ``n_negatives``
        rows per positive.

        DESIGN.md section 19c, ``objective='pairwise'`` only:

        * ``sampler='warp'``: per triple the device tries up to ``n_candidates`` admissible draws
          and trains against the first whose score exceeds ``s+ - margin``, weighted by
          ``log(max(1, A_b // N))`` (``N`` trials, ``A_b`` admissible candidates of the context);
          a triple without a violator has weight 0 for that epoch.
        * ``proposal``: the distribution of the device samplers' draws -- ``None`` (uniform),
          ``'popularity'`` (``(stored count of the candidate's column of interactions + 1) **
          proposal_power``) or ``C`` weights; quantised by ``quantise_proposal``.  Not with
          ``sampler='host'``.
        * ``sample_weight``: a confidence weight ``>= 0`` per positive -- with ``interactions``
          ``'data'`` (its stored values) or ``nnz`` values in canonical CSR order; with
          ``triples`` one value per triple.  It multiplies the triple's loss and gradient.

        The mean loss of the stopping rule stays ``sum_loss / m`` with ``m`` the number of
        triples, not the weight sum."""
        self._check_config()
        if objective not in OBJECTIVES:
            raise ValueError("objective %r is not supported. Choose from %s."
                             % (objective, list(OBJECTIVES)))
        listwise = objective != "pairwise"
        if listwise:
            check_lists(triples, n_negatives, objective)
        if sampler not in SAMPLERS:
            raise ValueError("sampler %r is not supported. Choose from %s."
                             % (sampler, list(SAMPLERS)))
        if (interactions is None) == (triples is None):
            raise ValueError("exactly one of interactions and triples must be given")
        if sampler != "host" and triples is not None:
            raise ValueError("sampler=%r draws the negatives on the device: give interactions, "
                             "not triples" % (sampler,))
        if int(n_candidates) != n_candidates or n_candidates < 1:
            raise ValueError("n_candidates must be an integer >= 1, got %r" % (n_candidates,))
        if listwise and (sampler == "warp" or sample_weight is not None):
            raise ValueError("sampler='warp' and sample_weight need objective='pairwise', got %r"
                             % (objective,))
        if sampler == "host" and proposal is not None:
            raise ValueError("proposal applies to the device samplers ('uniform', 'dynamic', "
                             "'warp'), not to sampler='host'")
        if sampler == "warp" and not np.isfinite(margin):
            raise ValueError("margin must be finite, got %r" % (margin,))
        Xa, Za = _prepare_pairs(self, X, Z)
        B, C = Xa.shape[0], Za.shape[0]
        n_features = Xa.shape[1]
        forbidden = None
        cum = None
        if interactions is not None:
            if not sp.issparse(interactions):
                interactions = sp.csr_matrix(np.asarray(interactions))
            stored = interactions
            interactions = _pattern(interactions, B, C, "interactions")
            if isinstance(sample_weight, str):
                if sample_weight != "data":
                    raise ValueError("sample_weight %r is not supported: 'data' or an array"
                                     % (sample_weight,))
                stored = sp.csr_matrix(stored, dtype=np.double, copy=True)
                stored.sum_duplicates()
                stored.sort_indices()
                sample_weight = stored.data
            if isinstance(proposal, str):
                if proposal != "popularity":
                    raise ValueError("proposal %r is not supported: None, 'popularity' or %d "
                                     "weights" % (proposal, C))
                proposal = popularity_weights(interactions, proposal_power)
            if proposal is not None:
                cum = proposal_cum(quantise_proposal(proposal, C))
            sample_weight = _check_weights(sample_weight, interactions.nnz, "stored entry of "
                                           "interactions")
            if interactions.nnz == 0:
                raise ValueError("interactions has no stored entry")
            if exclude is not None:
                exclude = _pattern(exclude, B, C, "exclude")
            if sampler != "host":
                if int(n_negatives) != n_negatives or n_negatives < 1:
                    raise ValueError("n_negatives must be an integer >= 1, got %r"
                                     % (n_negatives,))
                if interactions.nnz * int(n_negatives) >= 2 ** 31:
                    raise ValueError("%d triples: the triple list is limited to 2**31 - 1 rows"
                                     % (interactions.nnz * int(n_negatives)))
                interactions, forbidden = _forbidden(interactions, exclude, B, C)
        else:
            triples = check_triples(triples, B, C)
            if triples.shape[0] == 0:
                raise ValueError("triples is empty")
            sample_weight = _check_weights(sample_weight, triples.shape[0], "triple")
        rng = check_random_state(self.random_state)
        if not (self.warm_start and hasattr(self, "w_")):
            self.w_ = np.zeros(n_features, dtype=np.double)
        n_orders = self.degree - 1 if self.fit_lower == "explicit" else 1
        if not (self.warm_start and hasattr(self, "P_")):
            self.P_ = 0.01 * rng.randn(n_orders, self.n_components, n_features)
        if not (self.warm_start and hasattr(self, "lams_")):
            if self.init_lambdas == "ones":
                self.lams_ = np.ones(self.n_components)
            elif self.init_lambdas == "random_signs":
                self.lams_ = np.sign(rng.randn(self.n_components))
            else:
                raise ValueError("Lambdas must be initialized as ones (init_lambdas='ones') or "
                                 "as random +/- 1 (init_lambdas='random_signs').")
        if np.unique(np.abs(self.lams_)) != np.array([1.0]):
            raise ValueError("Lambdas must be +1 or -1.")
        if self.P_.shape != (n_orders, self.n_components, n_features) or \
                self.w_.shape != (n_features,):
            raise ValueError("warm_start: P_ / w_ do not fit this data and configuration")
        if not (self.warm_start and hasattr(self, "it_")):
            self.it_ = 1
        S = sp.vstack([Xa, Za], format="csr")
        S.sort_indices()
        if self.batch_size == "auto":
            batch_size = max(1, int(S.shape[0] * n_features / max(S.nnz, 1)))
        else:
            batch_size = self.batch_size
        engine = self._new_engine()
        try:
            engine.set_data(S, np.zeros(S.shape[0]))
            self.P_ = np.ascontiguousarray(self.P_, dtype=np.double)
            self.w_ = np.ascontiguousarray(self.w_, dtype=np.double)
            engine.set_params(self.P_, self.w_, self.lams_)
            engine.configure("psgd", self.loss, self.regularizer, self.degree)
            self._adagrad_begin(engine, self.P_.shape)
            if sampler == "host" and sample_weight is not None:
                lists = epoch_triples(rng, self.max_iter, interactions, triples, n_negatives,
                                      resample, self.shuffle, exclude, weights=sample_weight)
            elif sampler == "host":
                lists = (epoch_lists if listwise else epoch_triples)(
                    rng, self.max_iter, interactions, triples, n_negatives, resample,
                    self.shuffle, exclude)
            else:
                engine.psgd_pairs_set_sampler(B, C, interactions, forbidden)
                if cum is not None:
                    engine.psgd_pairs_set_proposal(cum)
                if sample_weight is not None:
                    engine.psgd_pairs_set_positive_weights(sample_weight)
                lists = self._device_lists(engine, rng, interactions.nnz * int(n_negatives),
                                           int(n_negatives),
                                           1 if sampler == "uniform" else int(n_candidates),
                                           resample, listwise,
                                           float(margin) if sampler == "warp" else None)
            converged, self.n_iter_ = self._fit_pairs(engine, B, batch_size, lists,
                                                      objective, int(n_negatives))
        finally:
            engine.close()
        return self._finish_fit(converged)

    def _device_lists(self, engine, rng, m, n_negatives, n_candidates, resample,
                      listwise=False, warp_margin=None):
        """per epoch: have the device draw the epoch's negatives (before the first epoch and,
        with ``resample``, before every later one) and yield the number of resident triples;
        ``listwise``: the triples stay grouped and ``(m, visiting order of the lists or None)``
        is yielded; ``warp_margin``: the WARP sampler with that margin and ``n_candidates``
        trials"""
        seed = rng.randint(0, 2 ** 31 - 1)
        list_order = None
        for ep in range(self.max_iter):
            if listwise:
                if ep == 0 or resample:
                    list_order = rng.permutation(m // n_negatives) if self.shuffle else None
                    engine.psgd_pairs_sample(self.degree, n_negatives, n_candidates,
                                             64 * n_candidates, seed, ep, None,
                                             want_triples=False, want_scores=False)
                yield m, list_order
                continue
            if ep == 0 or resample:
                order = rng.permutation(m) if self.shuffle else None
                if warp_margin is not None:
                    engine.psgd_pairs_sample_warp(self.degree, n_negatives, n_candidates,
                                                  64 * n_candidates, warp_margin, seed, ep,
                                                  order, want=False)
                else:
                    engine.psgd_pairs_sample(self.degree, n_negatives, n_candidates,
                                             64 * n_candidates, seed, ep, order,
                                             want_triples=False, want_scores=False)
            yield m

    def _fit_pairs(self, engine, B, batch_size, lists, objective="pairwise", n_negatives=1):
        """the loop of ``_fit_psgd`` over the epochs' triple lists: (m, 3) arrays to upload
        (context / candidate numbering), or the size of the list the device sampler left (a list
        objective: with the visiting order of its lists); ``m`` counts the training items"""
        converged = False
        no_improvement_count = 0
        best_loss = np.inf
        epoch = 0
        step = (self.degree, self.alpha, self.beta, self.gamma, self.eta0, self._base_rate(),
                self.power_t, batch_size)
        for epoch, t in enumerate(lists):
            if objective != "pairwise" and isinstance(t, np.ndarray):
                m = t.shape[0] // n_negatives
                stacked = t + np.array([0, B, B], dtype=np.int32)  # rows of [X; Z]
                sum_loss, self.it_ = engine.psgd_lists_epoch(
                    *step, stacked, n_negatives, objective, self.fit_linear, self.it_)
            elif objective != "pairwise":
                m = t[0] // n_negatives
                sum_loss, self.it_ = engine.psgd_lists_epoch_sampled(
                    *step, n_negatives, objective, self.fit_linear, self.it_, list_order=t[1])
            elif isinstance(t, tuple):  # (triples, a weight per triple)
                m = t[0].shape[0]
                stacked = t[0] + np.array([0, B, B], dtype=np.int32)  # rows of [X; Z]
                sum_loss, self.it_ = engine.psgd_pairs_epoch_weighted(
                    *step, stacked, t[1], self.fit_linear, self.it_)
            elif isinstance(t, np.ndarray):
                m = t.shape[0]
                stacked = t + np.array([0, B, B], dtype=np.int32)  # rows of [X; Z]
                sum_loss, self.it_ = engine.psgd_pairs_epoch(
                    self.degree, self.alpha, self.beta, self.gamma, self.eta0,
                    self._base_rate(), self.power_t, batch_size, stacked, self.fit_linear,
                    self.it_)
            else:
                m = t
                sum_loss, self.it_ = engine.psgd_pairs_epoch_sampled(
                    self.degree, self.alpha, self.beta, self.gamma, self.eta0,
                    self._base_rate(), self.power_t, batch_size, self.fit_linear, self.it_)
            if (self.callback is not None) and epoch % self.n_calls == 0:
                if callback_needs_params(self.callback):
                    self._sync_params(engine)  # P_ and w_ as they stand after this epoch
                if self.callback(self) is not None:
                    break
            sum_loss /= m
            if self.verbose:
                print(f"Epoch {epoch+1} loss {sum_loss}")
            if sum_loss > (best_loss - self.tol):
                no_improvement_count += 1
            else:
                no_improvement_count = 0
            if sum_loss < best_loss:
                best_loss = sum_loss
            if no_improvement_count >= self.n_iter_no_change:
                if self.verbose:
                    print(f"Converged at iteration {epoch+1}")
                converged = True
                break
        self._sync_params(engine)
        self._adagrad_end(engine)
        return converged, epoch

    def sample_negatives(self, X, Z, interactions, n_negatives=1, n_candidates=8, exclude=None,
                         random_state=None):
        """Hard negatives under the fitted model, drawn and scored on the device
        (``spfm_psgd_pairs_sample``): for every stored ``(b, c+)`` of
        ``interactions``, ``n_negatives`` times the highest-scored of ``n_candidates`` admissible
        candidates (stored neither in row ``b`` of ``interactions`` nor of ``exclude``).  Returns
        ``(triples, scores)``: ``(m, 3)`` int32 rows ``(b, c+, c-)`` in context / candidate
        numbering and the chosen candidates' scores (zeros for ``n_candidates == 1``).  The seed
        is ``check_random_state(random_state).randint(0, 2**31 - 1)``, the epoch key 0."""
        if not hasattr(self, "P_"):
            raise NotFittedError("Estimator not fitted.")
        self._check_config()
        if int(n_negatives) != n_negatives or n_negatives < 1:
            raise ValueError("n_negatives must be an integer >= 1, got %r" % (n_negatives,))
        if int(n_candidates) != n_candidates or n_candidates < 1:
            raise ValueError("n_candidates must be an integer >= 1, got %r" % (n_candidates,))
        Xa, Za = _prepare(self, X, Z)
        B, C = Xa.shape[0], Za.shape[0]
        if not sp.issparse(interactions):
            interactions = sp.csr_matrix(np.asarray(interactions))
        I, F = _forbidden(interactions, exclude, B, C)
        if I.nnz == 0:
            raise ValueError("interactions has no stored entry")
        if I.nnz * int(n_negatives) >= 2 ** 31:
            raise ValueError("%d triples: the triple list is limited to 2**31 - 1 rows"
                             % (I.nnz * int(n_negatives)))
        seed = check_random_state(random_state).randint(0, 2 ** 31 - 1)
        S = sp.vstack([Xa, Za], format="csr")
        S.sort_indices()
        engine = self._new_engine()
        try:
            engine.set_data(S, np.zeros(S.shape[0]))
            engine.set_params(np.ascontiguousarray(self.P_, dtype=np.double), self.w_, self.lams_)
            engine.configure("psgd", self.loss, self.regularizer, self.degree)
            engine.psgd_pairs_set_sampler(B, C, I, F)
            _, t, sc = engine.psgd_pairs_sample(self.degree, int(n_negatives), int(n_candidates),
                                                64 * int(n_candidates), seed, 0)
        finally:
            engine.close()
        return t - np.array([0, B, B], dtype=np.int32), sc

    def pairwise_loss(self, X, Z, triples):
        """``(mean loss, share of triples with margin > 0)`` of the fitted model on the triples
        ``(b, c+, c-)`` (context / candidate numbering), on the device
        (``spfm_psgd_pairs_eval``).  Like the fit the margin sums every order of ``P_``."""
        if not hasattr(self, "P_"):
            raise NotFittedError("Estimator not fitted.")
        self._check_config()
        Xa, Za = _prepare(self, X, Z)
        t = check_triples(triples, Xa.shape[0], Za.shape[0])
        if t.shape[0] == 0:
            raise ValueError("triples is empty")
        S = sp.vstack([Xa, Za], format="csr")
        S.sort_indices()
        engine = self._new_engine()
        try:
            engine.set_data(S, np.zeros(S.shape[0]))
            engine.set_params(np.ascontiguousarray(self.P_, dtype=np.double), self.w_, self.lams_)
            engine.configure("psgd", self.loss, self.regularizer, self.degree)
            sum_loss, n_ordered = engine.psgd_pairs_eval(
                self.degree, self.fit_linear, t + np.array([0, Xa.shape[0], Xa.shape[0]],
                                                           dtype=np.int32))
        finally:
            engine.close()
        return sum_loss / t.shape[0], n_ordered / t.shape[0]

    def list_loss(self, X, Z, triples, n_negatives, objective="softmax"):
        """``(mean loss per list, share of lists whose positive scores above all of its
        negatives)`` of the fitted model on the grouped triples -- ``n_negatives`` rows
        ``(b, c+, c-)`` per positive, context / candidate numbering -- on the device
        (``spfm_psgd_lists_eval``); ``objective``: ``'softmax'`` or ``'list'`` (the estimator's
        ``loss``)."""
        if not hasattr(self, "P_"):
            raise NotFittedError("Estimator not fitted.")
        self._check_config()
        check_lists(triples, n_negatives, objective)
        Xa, Za = _prepare(self, X, Z)
        t = check_triples(triples, Xa.shape[0], Za.shape[0])
        if t.shape[0] == 0:
            raise ValueError("triples is empty")
        S = sp.vstack([Xa, Za], format="csr")
        S.sort_indices()
        engine = self._new_engine()
        try:
            engine.set_data(S, np.zeros(S.shape[0]))
            engine.set_params(np.ascontiguousarray(self.P_, dtype=np.double), self.w_, self.lams_)
            engine.configure("psgd", self.loss, self.regularizer, self.degree)
            sum_loss, n_first = engine.psgd_lists_eval(
                self.degree, self.fit_linear,
                t + np.array([0, Xa.shape[0], Xa.shape[0]], dtype=np.int32), int(n_negatives),
                objective)
        finally:
            engine.close()
        q = t.shape[0] // int(n_negatives)
        return sum_loss / q, n_first / q

    def decision_function(self, rows):
        """The model output of every row of ``rows`` (n, d), e.g. of ``x_b + z_c``."""
        return self._predict(rows)
