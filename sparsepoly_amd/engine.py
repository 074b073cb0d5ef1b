"""Python face of one ``spfm_handle`` (include/spfm.h): NumPy in, NumPy out.

The methods map one-to-one onto the reference calls they replace
(``sparsepoly/sparse_factorization_machines.py`` epoch drivers):

=====================  =====================================================
``set_data``           ``get_dataset(X, 'fortran')`` + ``row_norms`` (:406-409)
``init_pred``          ``_get_output(X)`` (:408, :437-451)
``cd_linear_epoch``    ``cd_linear._cd_linear_epoch`` (optimizer/cd_linear.py:8-33)
``pcd_epoch``          ``pcd.pcd_epoch`` (optimizer/pcd.py:71-137)
``pbcd_epoch``         ``pbcd.pbcd_epoch`` (optimizer/pbcd.py:82-148)
``predict``            ``_predict`` (:453-458)
=====================  =====================================================
"""
import collections
import contextlib
import ctypes as C
import threading

import numpy as np
import scipy.sparse as sp

from . import _capi


class SpfmError(RuntimeError):
    pass


def canonical_csc(X):
    """CSC with sorted, duplicate-free row indices, float64.  Dense input is
    converted entry-wise (the reference's FortranDataset, dataset.py:39-57, also
    visits explicit zeros; they contribute exact zeros to every sum and update)."""
    if sp.issparse(X):
        Xc = sp.csc_matrix(X, dtype=np.float64, copy=True)
        Xc.sum_duplicates()
        Xc.sort_indices()
    else:
        Xc = sp.csc_matrix(np.asarray(X, dtype=np.float64))
        Xc.sort_indices()
    return Xc


def _stream_arrays(kind, d, nnz, G, nb, NG):
    """Zeroed arrays of the sizes spfm.h gives for the tables of a stream of ``kind``."""
    nsp = {"rowblock": G * nb * 65, "relaxed": G * nb * 65, "pbcd": G * nb * (NG + 1),
           "wide": G * (d + nb)}[kind] + 1
    out = dict(sp=np.zeros(nsp, dtype=np.int32), src=np.zeros(nnz, dtype=np.int32))
    if kind in ("rowblock", "relaxed"):
        out["lmask"] = np.zeros(G * nb * 2, dtype=np.uint32)
    else:
        out["flags"] = np.zeros(nnz, dtype=np.uint8)
    if kind == "pbcd":
        out["tab"] = np.zeros(G * max(nb, 1) * 64, dtype=np.uint8)
    return out


def _stream_ptrs(t):
    """The five table pointers of spfm_stream_build / spfm_debug_stream_tables (NULL = none)."""
    def ptr(name, ctype):
        return t[name].ctypes.data_as(ctype) if name in t else None
    return (ptr("sp", _capi._ip), ptr("src", _capi._ip), ptr("flags", _capi._bp),
            ptr("lmask", _capi._up), ptr("tab", _capi._bp))


def stream_build(kind, n_rows, indptr, indices, order, batch_ptr, groups, long_thresh=48, NG=16,
                 balance=True, skip=None):
    """``spfm_stream_build``: the host form of the entry-stream builders on a canonical CSC
    structure -- no handle, no device.  ``kind``: 'rowblock' (``skip``: the relaxed runs' form),
    'pbcd' or 'wide'.  Returns a dict of the tables (include/spfm.h): ``sp``, ``src`` and
    ``lmask`` (row-block kinds) or ``flags`` (+ ``tab`` for 'pbcd'), cut to ``n_entries``."""
    lib = _capi.load()
    ipa, ipp = _capi.i64(indptr)
    ixa, ixp = _capi.i32(indices)
    oa, op = _capi.i32(order)
    ba, bp = _capi.i32(batch_ptr)
    d, nb, nnz = oa.shape[0], ba.shape[0] - 1, int(ipa[-1])
    if ipa.shape[0] != d + 1 or ixa.shape[0] != nnz:
        raise ValueError("stream_build: indptr / indices / order do not fit together")
    if skip is not None:
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        if skip.shape[0] != nnz:
            raise ValueError("stream_build: skip needs one byte per entry")
    t = _stream_arrays(kind, d, nnz, int(groups), nb, int(NG))
    ne = C.c_int64()
    rc = lib.spfm_stream_build(
        _capi.STREAMS[kind], int(n_rows), d, ipp, ixp, op, bp, nb, int(groups), int(long_thresh),
        int(NG), int(bool(balance)), None if skip is None else skip.ctypes.data_as(_capi._bp),
        *(_stream_ptrs(t) + (C.byref(ne),)))
    if rc != 0:
        raise ValueError("spfm_stream_build failed (%d): bad arguments" % rc)
    t["n_entries"] = ne.value
    for name in ("src", "flags"):
        if name in t:
            t[name] = t[name][:ne.value]
    return t


# Engines created inside `co_tenancy(n)` -- or by the worker threads of one
# `fit_concurrently` call -- announce that n of them train side by side on one GPU
# (sparsepoly_amd/concurrent.py): every persistent pass keeps to 1/n of the CUs.  The state of
# such a call is a `Tenancy` object bound to the THREADS that take part in it (thread-local), so
# two calls that overlap in time from different threads do not see each other's shares.
_TLS = threading.local()
_SHARED_LOCK = threading.Lock()
_SCHEDULE_LRU = collections.OrderedDict()
_SCHEDULE_LRU_SIZE = 8
_SCHEDULE_STATS = {"hits": 0, "misses": 0}


class Tenancy(object):
    """What the fits of ONE concurrent call share: the number of tenants per device, the device
    a worker thread fits on (``devices=[...]`` fan-out), and -- one data set for all -- the
    coloured schedule and the device data image (first come computes / uploads, the others
    install / attach)."""

    def __init__(self, n, share_schedules=False, share_data=False, device=None):
        self.n = max(1, int(n))
        self.schedules = {} if share_schedules else None
        self.images = {} if share_data else None  # key -> {"done": Event, "keeper": HipEngine}
        self.device = device
        self.lock = threading.Lock()

    def on_device(self, device):
        """The same call's state as seen by a worker bound to `device` (shared caches are per
        device: a schedule object is portable, a device image is not)."""
        t = Tenancy.__new__(Tenancy)
        t.n, t.lock, t.device = self.n, self.lock, device
        t.schedules, t.images = self.schedules, self.images
        return t

    def close(self):
        if self.images:
            for ent in self.images.values():
                k = ent.get("keeper")
                if k is not None:
                    k.close()
            self.images.clear()


def current_tenancy():
    return getattr(_TLS, "tenancy", None)


def bind_tenancy(tenancy):
    """Bind `tenancy` (or None) to the calling thread; returns what was bound before."""
    old = getattr(_TLS, "tenancy", None)
    _TLS.tenancy = tenancy
    return old


def structure_key(X):
    """Content hash of a sparse matrix's STRUCTURE (shape, format, indptr, indices): what a
    colouring depends on.  ~0.05 s for 50 M entries."""
    try:
        import xxhash

        h = xxhash.xxh3_64()
    except Exception:  # pragma: no cover - xxhash is optional
        import hashlib

        h = hashlib.blake2b(digest_size=8)
    for a in (X.indptr, X.indices):
        h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
    return (X.format, X.shape, int(X.nnz), h.hexdigest())


class co_tenancy(object):
    """``with co_tenancy(n):`` -- engines created by THIS thread inside the block share the device
    with n - 1 others (per-call state: see Tenancy)."""

    def __init__(self, n, share_schedules=False, share_data=False, device=None):
        self.tenancy = Tenancy(n, share_schedules, share_data, device)

    def __enter__(self):
        if self.tenancy.n > 1:
            _capi.ensure_hw_queues(self.tenancy.n)
        self._old = bind_tenancy(self.tenancy)
        return self.tenancy

    def __exit__(self, *exc):
        bind_tenancy(self._old)
        self.tenancy.close()
        return False


def shared_schedule(key, compute, install):
    """Inside a concurrent call that shares schedules: ``compute()`` (-> order, Schedule) runs in
    the first thread that asks for ``key``; every other thread waits for it and calls
    ``install(schedule)`` (-> order).  Outside such a call the process-wide memory of schedules
    is consulted instead."""
    ten = current_tenancy()
    cache = ten.schedules if ten is not None else None
    if cache is None:
        # one fit at a time: a small process-wide memory of coloured schedules, so that a second
        # fit on the same matrix in the same visiting order (a grid search, a restart) does not
        # colour it again (0.5 s on BASELINE config 2, 7 s on configs[4])
        with _SHARED_LOCK:
            sched = _SCHEDULE_LRU.get(key)
            if sched is not None:
                _SCHEDULE_LRU.move_to_end(key)
            _SCHEDULE_STATS["hits" if sched is not None else "misses"] += 1
        if sched is not None:
            return install(sched)
        order, sched = compute()
        with _SHARED_LOCK:
            _SCHEDULE_LRU[key] = sched
            while len(_SCHEDULE_LRU) > _SCHEDULE_LRU_SIZE:
                _SCHEDULE_LRU.popitem(last=False)
        return order
    with ten.lock:
        entry = cache.get(key)
        leader = entry is None
        if leader:
            entry = cache[key] = {"done": threading.Event(), "sched": None}
    if leader:
        try:
            order, entry["sched"] = compute()
        finally:
            entry["done"].set()     # on an error the followers compute for themselves
        return order
    entry["done"].wait()
    if entry["sched"] is None:
        return compute()[0]
    return install(entry["sched"])


def data_key(X, precision, device):
    """Content hash of a sparse matrix (structure AND values) + what else decides its device
    image."""
    try:
        import xxhash

        h = xxhash.xxh3_64()
    except Exception:  # pragma: no cover - xxhash is optional
        import hashlib

        h = hashlib.blake2b(digest_size=8)
    for a in (X.indptr, X.indices, X.data):
        h.update(memoryview(np.ascontiguousarray(a)).cast("B"))
    return (X.format, X.shape, int(X.nnz), h.hexdigest(), precision, int(device))


def shared_set_data(engine, X, y):
    """``engine.set_data(X, y)`` -- or, inside a concurrent call on ONE data set, attach to the
    device image the first fit of that call uploaded (Tenancy.images; kept alive by a keeper
    handle until the call ends)."""
    ten = current_tenancy()
    if ten is None or ten.images is None or not sp.issparse(X):
        engine.set_data(X, y)
        return False
    key = data_key(X, engine.precision, engine.device)
    with ten.lock:
        entry = ten.images.get(key)
        leader = entry is None
        if leader:
            entry = ten.images[key] = {"done": threading.Event(), "keeper": None}
    if leader:
        try:
            engine.set_data(X, y)
            keeper = HipEngine(engine.device, engine.precision)
            keeper.share_data(engine)
            entry["keeper"] = keeper
        finally:
            entry["done"].set()  # on an error the followers upload for themselves
        return False
    entry["done"].wait()
    if entry["keeper"] is None:
        engine.set_data(X, y)
        return False
    engine.share_data(entry["keeper"], y)
    return True


def hw_queue_report():
    """How many hardware queues the HIP runtime of this process maps streams onto, as far as the
    environment tells (GPU_MAX_HW_QUEUES is read when the runtime initialises; default 4).  More
    concurrent fits than queues share queues, and two persistent passes on one queue run one
    after the other (independent fits side by side)."""
    import os

    val = os.environ.get("GPU_MAX_HW_QUEUES")
    return {"GPU_MAX_HW_QUEUES": int(val) if val and val.isdigit() else None,
            "runtime_default": 4,
            "set_by_package": bool(_capi.QUEUES_SET_BY_PACKAGE),
            "hip_initialised_before_import": bool(_capi.HIP_INITIALISED_BEFORE_IMPORT)}


class HipEngine(object):
    def __init__(self, device=0, precision="f32"):
        if precision not in _capi.DTYPES:
            raise ValueError("precision must be 'f32' or 'f64'")
        self._lib = _capi.load()
        h = C.c_void_p()
        rc = self._lib.spfm_create(C.byref(h), int(device), _capi.DTYPES[precision])
        if rc != 0:
            msg = self._lib.spfm_last_error(None).decode()
            raise SpfmError("spfm_create failed: %s" % msg)
        self._h = h
        self.precision = precision
        self.n = self.d = self.nnz = self.k = self.n_orders = None
        self.order = None
        self.n_batches = None
        self.device = int(device)
        ten = current_tenancy()
        self.tenants = ten.n if ten is not None else 1
        if self.tenants > 1:
            self.set_option("co_tenants", self.tenants)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.spfm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == 0:
            return
        msg = self._lib.spfm_last_error(self._h).decode()
        if rc == _capi.SPFM_ERR_INVALID:
            raise ValueError(msg)
        if rc == _capi.SPFM_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise SpfmError(msg)

    @property
    def device_name(self):
        buf = C.create_string_buffer(128)
        self._check(self._lib.spfm_device_name(self._h, buf, 128))
        return buf.value.decode()

    # ------------------------------------------------------------------ data
    def set_data(self, X, y):
        if sp.isspmatrix_csr(X) and X.has_canonical_format:
            # CSR input: no scipy tocsc(); the library transposes on host threads
            n, d = X.shape
            keep = [_capi.i64(X.indptr), _capi.i32(X.indices), _capi.f64(X.data), _capi.f64(y)]
            if keep[3][0].shape[0] != n:
                raise ValueError("y has %d entries, X has %d rows" % (keep[3][0].shape[0], n))
            self._check(self._lib.spfm_set_data_csr(self._h, n, d, keep[0][1], keep[1][1],
                                                    keep[2][1], keep[3][1]))
            self.n, self.d, self.nnz = n, d, int(keep[0][0][-1])
            return
        Xc = X if (sp.isspmatrix_csc(X) and X.has_canonical_format) else canonical_csc(X)
        n, d = Xc.shape
        self._keep = [_capi.i64(Xc.indptr), _capi.i32(Xc.indices), _capi.f64(Xc.data),
                      _capi.f64(y)]
        if self._keep[3][0].shape[0] != n:
            raise ValueError("y has %d entries, X has %d rows" % (self._keep[3][0].shape[0], n))
        self._check(self._lib.spfm_set_data_csc(
            self._h, n, d, self._keep[0][1], self._keep[1][1], self._keep[2][1],
            self._keep[3][1]))
        self.n, self.d, self.nnz = n, d, int(self._keep[0][0][-1])
        self._keep = None

    def share_data(self, src, y=None):
        """Train on the device image of the matrix that engine ``src`` holds (no upload, no
        second copy in HBM); ``y``: this engine's own targets, default ``src``'s."""
        if y is None:
            yp = None
        else:
            ya, yp = _capi.f64(y)
            if ya.shape[0] != src.n:
                raise ValueError("y has %d entries, X has %d rows" % (ya.shape[0], src.n))
        self._check(self._lib.spfm_share_data(self._h, src._h, yp))
        self.n, self.d, self.nnz = src.n, src.d, src.nnz

    def set_sample_weight(self, sample_weight):
        """One weight per row of this engine's training data (``spfm_set_sample_weight``,
        DESIGN.md section 20); ``None`` clears.  New data (``set_data`` / ``share_data``) clears
        them too."""
        if sample_weight is None:
            self._check(self._lib.spfm_set_sample_weight(self._h, None, 0))
            return
        wa, wp = _capi.f64(sample_weight)
        self._check(self._lib.spfm_set_sample_weight(self._h, wp, wa.shape[0]))

    def sample_weight_set(self):
        flag = C.c_int()
        self._check(self._lib.spfm_get_sample_weight(self._h, C.byref(flag), None))
        return bool(flag.value)

    def sample_weight_sum(self):
        """Sum of the weights; the row count when none are set."""
        out = C.c_double()
        self._check(self._lib.spfm_get_sample_weight(self._h, None, C.byref(out)))
        return out.value

    def set_params(self, P, w, lams):
        P = np.ascontiguousarray(P, dtype=np.float64)
        if P.ndim != 3:
            raise ValueError("P must be (n_orders, n_components, n_features)")
        n_orders, k, d = P.shape
        Pa, Pp = _capi.f64(P)
        wa, wp = _capi.f64(w)
        la, lp = _capi.f64(lams)
        if wa.shape[0] != d or la.shape[0] != k:
            raise ValueError("w / lams shapes do not match P")
        self._check(self._lib.spfm_set_params(self._h, n_orders, k, d, Pp, wp, lp))
        self.n_orders, self.k, self.d = n_orders, k, d
        self.n_candidates = None  # the library forgets the candidate towers with the parameters

    def get_params(self, P=None, w=None, skip_P=False):
        """Copy the live device state into P (n_orders, k, d) and w (d), in place when
        arrays are given.  ``skip_P`` leaves P untouched (pbcd callbacks)."""
        if P is None and not skip_P:
            P = np.empty((self.n_orders, self.k, self.d))
        if w is None:
            w = np.empty(self.d)
        assert w.flags.c_contiguous and w.dtype == np.float64
        Pp = None
        if not skip_P:
            assert P.flags.c_contiguous and P.dtype == np.float64
            Pp = P.ctypes.data_as(_capi._dp)
        self._check(self._lib.spfm_get_params(self._h, Pp, w.ctypes.data_as(_capi._dp)))
        return P, w

    def configure(self, solver, loss, regularizer, degree):
        if solver not in _capi.SOLVERS:
            raise ValueError("Solver %s is not supported." % solver)
        self._check(self._lib.spfm_configure(
            self._h, _capi.SOLVERS[solver], _capi.LOSSES[loss], _capi.REGULARIZERS[regularizer],
            int(degree)))

    def init_pred(self, degree, fit_linear, add_lower_deg2):
        self._check(self._lib.spfm_init_pred(self._h, int(degree), int(bool(fit_linear)),
                                             int(bool(add_lower_deg2))))

    def get_y_pred(self):
        out = np.empty(self.n)
        self._check(self._lib.spfm_get_y_pred(self._h, out.ctypes.data_as(_capi._dp)))
        return out

    def loss_sum(self):
        out = C.c_double()
        self._check(self._lib.spfm_loss_sum(self._h, C.byref(out)))
        return out.value

    def predict(self, X, degree, fit_linear, add_lower_deg2):
        Xr = sp.csr_matrix(X, dtype=np.float64)
        Xr.sum_duplicates()
        n = Xr.shape[0]
        if Xr.shape[1] != self.d:
            raise ValueError("X has %d features, the model has %d" % (Xr.shape[1], self.d))
        ia, ip = _capi.i64(Xr.indptr)
        ja, jp = _capi.i32(Xr.indices)
        da, dp = _capi.f64(Xr.data)
        out = np.zeros(n)
        self._check(self._lib.spfm_predict_csr(
            self._h, n, ip, jp, dp, int(degree), int(bool(fit_linear)),
            int(bool(add_lower_deg2)), out.ctypes.data_as(_capi._dp)))
        return out

    # --------------------------------- objective terms, held-out set (spfm.h, last section)
    OBJECTIVE_SLOTS = ("l2", "omega", "nnz", "active_features", "active_components")

    def objective_terms(self, order_idx, degree):
        """``spfm_objective_terms``: dict with ``l2`` (0.5 * sum of squares), ``omega`` (the
        configured regularizer of the block at ``degree``), ``nnz``, ``active_features`` and
        ``active_components`` of the LIVE block ``P[order_idx]`` (``order_idx = -1``: ``w``; then
        only ``l2`` and ``nnz`` are non-zero).  Nothing is copied to the host but eight doubles.

        ``omega`` equals the reference's ``regularizer.eval`` for five of the six regularizers.
        For ``omegacs`` it deviates on purpose: the reference's ``OmegaCS.eval`` reshapes its
        input instead of transposing it (``omegacs.py:22-39``), so for a non-square block it is
        not the function its own prox minimises; the value here is the prox cache's
        (``compute_cache_pbcd``, then ``_cache[degree]``)."""
        out = np.zeros(8)
        self._check(self._lib.spfm_objective_terms(self._h, int(order_idx), int(degree),
                                                   out.ctypes.data_as(_capi._dp)))
        return dict(l2=float(out[0]), omega=float(out[1]), nnz=int(out[2]),
                    active_features=int(out[3]), active_components=int(out[4]))

    def set_eval_data(self, X, y=None):
        """``spfm_set_eval_csr``: keep a held-out matrix (and its targets) on the device next to
        the training data; replaced by the next call."""
        Xr = sp.csr_matrix(X, dtype=np.float64)
        Xr.sum_duplicates()
        Xr.sort_indices()
        n, d = Xr.shape
        if self.d is not None and d != self.d:
            raise ValueError("X has %d features, the model has %d" % (d, self.d))
        ia, ip = _capi.i64(Xr.indptr)
        ja, jp = _capi.i32(Xr.indices)
        da, dp = _capi.f64(Xr.data)
        yp = None
        if y is not None:
            ya, yp = _capi.f64(y)
            if ya.shape[0] != n:
                raise ValueError("y has %d entries, X has %d rows" % (ya.shape[0], n))
        self._check(self._lib.spfm_set_eval_csr(self._h, n, d, ip, jp, dp, yp))
        self.n_eval, self._eval_has_y = n, y is not None

    def eval_loss(self, degree, fit_linear, add_lower_deg2, return_pred=False):
        """``spfm_eval_loss``: sum of the configured loss over the held-out set under the live
        parameters (None when the set has no targets); with ``return_pred`` the pair
        (loss sum, predictions)."""
        if getattr(self, "n_eval", None) is None:
            raise ValueError("eval_loss: call set_eval_data first")
        ls = C.c_double()
        lp = C.byref(ls) if self._eval_has_y else None
        pred, pp = None, None
        if return_pred:
            pred = np.zeros(self.n_eval)
            pp = pred.ctypes.data_as(_capi._dp)
        self._check(self._lib.spfm_eval_loss(self._h, int(degree), int(bool(fit_linear)),
                                             int(bool(add_lower_deg2)), lp, pp))
        val = ls.value if self._eval_has_y else None
        return (val, pred) if return_pred else val

    # ------------------------- selected interactions W = P_o^T diag(lams) P_o (spfm.h, last section)
    @contextlib.contextmanager
    def _interaction_features(self, n_features):
        """Restrict ONE stats / topk / list call to the features [0, n_features) (None: all): the
        handle's option is set for the call and restored with it, so nothing stays behind."""
        if n_features is None or n_features >= self.d:
            yield
            return
        old = self.get_option("interaction_features")
        self.set_option("interaction_features", int(n_features))
        try:
            yield
        finally:
            self.set_option("interaction_features", old)

    def release_interaction_scratch(self):
        """Free the device scratch the interaction calls keep between calls."""
        self.set_option("interaction_release", 1)

    def _interaction_stats_dict(self, entry, order_idx, tol):
        """The stats dictionary of ``spfm_interaction_stats`` / ``spfm_interaction3_stats``."""
        cnt = np.zeros(2, dtype=np.int64)
        sums = np.zeros(3)
        self._check(entry(self._h, int(order_idx), float(tol), cnt.ctypes.data_as(_capi._lp),
                          sums.ctypes.data_as(_capi._dp)))
        return dict(nnz=int(cnt[0]), active_features=int(cnt[1]), sum_sq=float(sums[0]),
                    sum_abs=float(sums[1]), max_abs=float(sums[2]))

    def _interaction_out(self, call, n_ids, size):
        """Runs ``call(ids_0, .., ids_{n_ids - 1}, vals, n_out)`` on arrays of ``size`` -> the
        ``n_out`` first of each."""
        arrs = [np.zeros(max(size, 1), dtype=np.int32) for _ in range(n_ids)]
        vals = np.zeros(max(size, 1))
        n = C.c_int64()
        self._check(call(*[a.ctypes.data_as(_capi._ip) for a in arrs],
                         vals.ctypes.data_as(_capi._dp), C.byref(n)))
        return tuple(a[:n.value].copy() for a in arrs) + (vals[:n.value].copy(),)

    def interaction_stats(self, order_idx, tol=0.0, n_features=None):
        """``spfm_interaction_stats``: dict ``nnz`` (pairs j < j' with ``|W| > tol``),
        ``active_features``, ``sum_sq``, ``sum_abs``, ``max_abs`` of the LIVE block
        (``n_features``: of its first features only)."""
        with self._interaction_features(n_features):
            return self._interaction_stats_dict(self._lib.spfm_interaction_stats, order_idx, tol)

    def interaction_topk(self, order_idx, K, n_features=None):
        """``spfm_interaction_topk``: ``(rows, cols, vals)`` of the K largest ``|W|`` among
        ``W != 0``, by ``|W|`` descending, then row, then column."""
        K = int(K)
        with self._interaction_features(n_features):
            return self._interaction_out(
                lambda *out: self._lib.spfm_interaction_topk(self._h, int(order_idx), K, *out),
                2, K)

    def interaction_list(self, order_idx, tol, capacity, n_features=None):
        """``spfm_interaction_list``: ``(rows, cols, vals)`` of every pair with ``|W| > tol``,
        sorted by (row, col).  ``ValueError`` naming the count when it exceeds ``capacity``."""
        capacity = int(capacity)
        with self._interaction_features(n_features):
            return self._interaction_out(
                lambda *out: self._lib.spfm_interaction_list(
                    self._h, int(order_idx), float(tol), capacity, *out), 2, capacity)

    def interaction_values(self, order_idx, rows, cols):
        """``spfm_interaction_values``: ``W[rows[q], cols[q]]`` (0 where the two ids are equal)."""
        ra, rp = _capi.i32(rows)
        ca, cp = _capi.i32(cols)
        if ra.ndim != 1 or ra.shape != ca.shape:
            raise ValueError("rows and cols must be 1-d arrays of one length")
        vals = np.zeros(ra.shape[0])
        self._check(self._lib.spfm_interaction_values(
            self._h, int(order_idx), ra.shape[0], rp, cp, vals.ctypes.data_as(_capi._dp)))
        return vals

    def interaction_block(self, order_idx, J, J2=None):
        """``spfm_interaction_block``: the dense ``W[J, J2]`` (``J2 = J`` by default), 0 where
        ``J[a] == J2[b]``; refused above ``SPFM_INTERACTION_BLOCK_MAX_BYTES``."""
        ja, jp = _capi.i32(J)
        j2a, j2p = (ja, jp) if J2 is None else _capi.i32(J2)
        if ja.ndim != 1 or j2a.ndim != 1:
            raise ValueError("J and J2 must be 1-d index arrays")
        if ja.shape[0] * j2a.shape[0] * 8 > _capi.INTERACTION_BLOCK_MAX_BYTES:
            raise ValueError("interaction_block: %d x %d doubles exceed the budget of %d bytes"
                             % (ja.shape[0], j2a.shape[0], _capi.INTERACTION_BLOCK_MAX_BYTES))
        out = np.zeros((ja.shape[0], j2a.shape[0]))
        self._check(self._lib.spfm_interaction_block(
            self._h, int(order_idx), ja.shape[0], jp, j2a.shape[0], j2p,
            out.ctypes.data_as(_capi._dp)))
        return out

    def interaction_degrees(self, order_idx, tol=0.0, n_features=None, cand_strip=0):
        """``spfm_interaction_degrees``: dict of arrays over the features in view, ``degree``
        (int64: partners ``j' != j`` with ``|W[j, j']| > tol``), ``sum_abs``, ``max_abs`` and
        ``strongest`` (int32: the smallest partner attaining ``max_abs``, -1 when it is 0).
        ``cand_strip`` (columns a workgroup walks) changes no result bit."""
        d = self.d or 0  # (no parameters yet: the entry refuses)
        n = d if n_features is None else min(int(n_features), d)
        deg = np.zeros(d, dtype=np.int64)
        sa, ma = np.zeros(d), np.zeros(d)
        st = np.full(d, -1, dtype=np.int32)
        with self._interaction_features(n_features):
            self._check(self._lib.spfm_interaction_degrees(
                self._h, int(order_idx), float(tol), int(cand_strip),
                deg.ctypes.data_as(_capi._lp), sa.ctypes.data_as(_capi._dp),
                ma.ctypes.data_as(_capi._dp), st.ctypes.data_as(_capi._ip)))
        return dict(degree=deg[:n].copy(), sum_abs=sa[:n].copy(), max_abs=ma[:n].copy(),
                    strongest=st[:n].copy())

    def interaction_partners(self, order_idx, J, K, among=None, by="abs", n_features=None,
                             row_slab=0, cand_strip=0):
        """``spfm_interaction_partners``: ``(ids (nJ, K) int32, vals (nJ, K), counts (nJ,) int32)``,
        the ``K`` strongest partners of every feature of ``J`` (None: every feature in view) among
        the features ``among = (lo, hi)`` (None: the view), by key descending (``by``: ``"abs"``
        ``|W|`` among ``W != 0``, ``"positive"`` ``W`` among ``W > 0``, ``"negative"`` ``-W`` among
        ``W < 0``), then id ascending.  ``vals`` is the signed ``W``; rows are padded with
        ``-1`` / ``0.0``.  ``row_slab`` / ``cand_strip`` change no result bit."""
        if by not in _capi.PARTNERS_BY:
            by_code = int(by) if isinstance(by, (int, np.integer)) else -1  # refused below
        else:
            by_code = _capi.PARTNERS_BY[by]
        d = self.d or 0  # (no parameters yet: the entry refuses)
        n = d if n_features is None else min(int(n_features), d)
        if J is None:
            nJ, jp = n, None
        else:
            ja, jp = _capi.i32(J)
            if ja.ndim != 1:
                raise ValueError("J must be a 1-d index array")
            nJ = ja.shape[0]
        K = int(K)
        lo, hi = (0, 0) if among is None else (int(among[0]), int(among[1]))
        if among is not None and hi <= 0:  # (0 means "the end of the view" to the C entry)
            raise ValueError("interaction_partners: among=(%d, %d) is empty" % (lo, hi))
        rows = nJ * K if 1 <= K <= _capi.INTERACTION_MAX_K else 0
        ids = np.full(max(rows, 1), -1, dtype=np.int32)
        vals = np.zeros(max(rows, 1))
        cnt = np.zeros(max(nJ, 1), dtype=np.int32)
        with self._interaction_features(n_features):
            self._check(self._lib.spfm_interaction_partners(
                self._h, int(order_idx), nJ, jp, K, lo, hi, by_code, int(row_slab),
                int(cand_strip), ids.ctypes.data_as(_capi._ip), vals.ctypes.data_as(_capi._dp),
                cnt.ctypes.data_as(_capi._ip)))
        return ids[:rows].reshape(nJ, K), vals[:rows].reshape(nJ, K), cnt[:nJ]

    # ------------------------- candidate ranking: scores and top-K of (context, candidate) pairs
    def _rank_csr(self, X, what):
        """Canonical CSR (sorted, duplicates summed) of the handle's width -> (matrix, pointers)"""
        Xr = sp.csr_matrix(X, dtype=np.float64)
        if not Xr.has_canonical_format:
            Xr = Xr.copy()
            Xr.sum_duplicates()
            Xr.sort_indices()
        if self.d is None:
            raise ValueError("%s: set_params first" % what)
        if Xr.shape[1] != self.d:
            raise ValueError("%s: the matrix has %d features, the model has %d"
                             % (what, Xr.shape[1], self.d))
        return Xr, (_capi.i64(Xr.indptr), _capi.i32(Xr.indices), _capi.f64(Xr.data))

    def rank_set_candidates(self, Z, degree, fit_linear, add_lower_deg2):
        """``spfm_rank_set_candidates``: build and keep the candidate towers of ``Z`` (C, d) under
        the handle's parameters.  ``degree`` -1: all-subsets."""
        Zr, (ia, ja, da) = self._rank_csr(Z, "rank_set_candidates")
        self._check(self._lib.spfm_rank_set_candidates(
            self._h, int(degree), int(bool(fit_linear)), int(bool(add_lower_deg2)), Zr.shape[0],
            ia[1], ja[1], da[1]))
        self.n_candidates = Zr.shape[0]

    def rank_scores(self, X):
        """``spfm_rank_scores``: the dense (B, C) scores of the contexts ``X`` against the resident
        candidates; refused above ``SPFM_RANK_SCORES_MAX_BYTES`` of result."""
        Xr, (ia, ja, da) = self._rank_csr(X, "rank_scores")
        C_ = getattr(self, "n_candidates", None)
        if C_ is None:
            raise ValueError("rank_scores: call rank_set_candidates first")
        if Xr.shape[0] * C_ * 8 > _capi.RANK_SCORES_MAX_BYTES:
            raise ValueError("rank_scores: %d x %d doubles exceed the budget of %d bytes"
                             % (Xr.shape[0], C_, _capi.RANK_SCORES_MAX_BYTES))
        out = np.zeros((Xr.shape[0], C_))
        self._check(self._lib.spfm_rank_scores(self._h, Xr.shape[0], ia[1], ja[1], da[1],
                                               out.ctypes.data_as(_capi._dp)))
        return out

    @staticmethod
    def _rank_pattern(pattern):
        """``(indptr, indices)`` of per-row candidate lists -> their int64 / int32 holders.  The
        arrays go to the library as they are; it checks them."""
        ptr, idx = pattern
        return _capi.i64(ptr), _capi.i32(idx)

    def rank_topk(self, X, K, exclude=None):
        """``spfm_rank_topk``: ``(idx, scores)`` of shape (B, min(K, C)), per row by score
        descending, then candidate index ascending.  ``K`` above ``SPFM_RANK_MAX_K``: ValueError.
        ``exclude``: ``(indptr, indices)``, per row the ascending candidate ids that are left out
        (``spfm_rank_topk_excl``); a row with fewer than K admissible candidates ends in -1 / NaN."""
        K = int(K)
        if K > _capi.RANK_MAX_K:
            raise ValueError("rank_topk: K = %d exceeds SPFM_RANK_MAX_K = %d (never answered "
                             "approximately)" % (K, _capi.RANK_MAX_K))
        Xr, (ia, ja, da) = self._rank_csr(X, "rank_topk")
        C_ = getattr(self, "n_candidates", None)
        if C_ is None:
            raise ValueError("rank_topk: call rank_set_candidates first")
        ko = max(min(K, C_), 1)
        idx = np.zeros((Xr.shape[0], ko), dtype=np.int32)
        val = np.zeros((Xr.shape[0], ko))
        k_out = C.c_int64()
        if exclude is None:
            self._check(self._lib.spfm_rank_topk(
                self._h, Xr.shape[0], ia[1], ja[1], da[1], K, idx.ctypes.data_as(_capi._ip),
                val.ctypes.data_as(_capi._dp), C.byref(k_out)))
        else:
            ep, ei = self._rank_pattern(exclude)
            self._check(self._lib.spfm_rank_topk_excl(
                self._h, Xr.shape[0], ia[1], ja[1], da[1], ep[1], ei[1], K,
                idx.ctypes.data_as(_capi._ip), val.ctypes.data_as(_capi._dp), C.byref(k_out)))
        assert k_out.value == ko
        return idx, val

    def rank_eval(self, X, targets, exclude=None):
        """``spfm_rank_eval``: ``(ranks, scores, n_eff)``.  ``targets`` and ``exclude`` are
        ``(indptr, indices)`` pairs, per context row ascending candidate ids; ``ranks`` (int32) and
        ``scores`` are aligned with the targets' ``indices``: the 0-based rank of each target among
        the candidates that are not excluded, and its score; ``n_eff`` (B,) = C minus the row's
        excluded candidates.  A target with a score that is not finite has rank -1."""
        Xr, (ia, ja, da) = self._rank_csr(X, "rank_eval")
        if getattr(self, "n_candidates", None) is None:
            raise ValueError("rank_eval: call rank_set_candidates first")
        tp, ti = self._rank_pattern(targets)
        ep, ei = self._rank_pattern(exclude) if exclude is not None else ((None, None),) * 2
        ranks = np.zeros(ti[0].shape[0], dtype=np.int32)
        scores = np.zeros(ti[0].shape[0])
        n_eff = np.zeros(Xr.shape[0], dtype=np.int32)
        self._check(self._lib.spfm_rank_eval(
            self._h, Xr.shape[0], ia[1], ja[1], da[1], tp[1], ti[1], ep[1], ei[1],
            ranks.ctypes.data_as(_capi._ip), scores.ctypes.data_as(_capi._dp),
            n_eff.ctypes.data_as(_capi._ip)))
        return ranks, scores, n_eff

    def rank_set_partition(self, row_slab=0, cand_strip=0):
        """``spfm_rank_set_partition``: context rows per slab and candidates per strip of the
        following ranking calls (0: the library's default).  No result bit depends on them."""
        self._check(self._lib.spfm_rank_set_partition(self._h, int(row_slab), int(cand_strip)))

    def rank_info(self):
        """``spfm_rank_info``: dict ``scratch_kib`` (device memory the ranking calls hold),
        ``device_ms`` (kernels of the last ``rank_scores`` / ``rank_topk`` / ``rank_eval``),
        ``row_slab``, ``cand_strip``."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._lib.spfm_rank_info(self._h, out.ctypes.data_as(_capi._lp)))
        return dict(scratch_kib=int((out[0] + 1023) // 1024), device_ms=out[1] / 1e3,
                    row_slab=int(out[2]), cand_strip=int(out[3]))

    def rank_release(self):
        """``spfm_rank_release``: free the ranking scratch and forget the candidates."""
        self._check(self._lib.spfm_rank_release(self._h))
        self.n_candidates = None

    # ------------------------- per-row attributions: values, gradients, row sums, top-K (spfm.h)
    def _explain_args(self, X, blocks, coef, fit_linear, what):
        """-> (canonical CSR, the ten leading arguments of the two entries, what keeps them alive)"""
        Xr, (ia, ja, da) = self._rank_csr(X, what)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.shape != (len(blocks), self.k, 7):
            raise ValueError("%s: coef must be (n_blocks, n_components, 7), got %r"
                             % (what, coef.shape))
        oa, op = _capi.i32(np.array([b[0] for b in blocks], dtype=np.int32))
        ga, gp = _capi.i32(np.array([b[1] for b in blocks], dtype=np.int32))
        ca, cp = _capi.f64(coef)
        args = (self._h, Xr.shape[0], ia[1], ja[1], da[1], len(blocks), op, gp, cp,
                int(bool(fit_linear)))
        return Xr, args, (ia, ja, da, oa, ga, ca)

    def explain(self, X, blocks, coef, fit_linear, mode="attribution", rowsum=True):
        """``spfm_explain_csr``: ``(vals, rowsum)`` for the canonical CSR form of ``X``: per stored
        entry (in the order of its ``data``) the attribution ``phi_ij`` or, with
        ``mode='gradient'``, ``df/dx_ij``; per row their sum (``None`` without ``rowsum``).
        ``blocks``: ``(order_idx, degree)`` pairs, ``coef`` (n_blocks, k, 7) their tables."""
        if mode not in _capi.EXPLAIN_MODES:
            raise ValueError("explain: mode must be 'attribution' or 'gradient', got %r" % (mode,))
        Xr, args, keep = self._explain_args(X, blocks, coef, fit_linear, "explain")
        vals = np.zeros(Xr.nnz)
        rs = np.zeros(Xr.shape[0]) if rowsum else None
        self._check(self._lib.spfm_explain_csr(
            *args, _capi.EXPLAIN_MODES[mode], vals.ctypes.data_as(_capi._dp),
            rs.ctypes.data_as(_capi._dp) if rowsum else None))
        return vals, rs

    def explain_topk(self, X, blocks, coef, fit_linear, K):
        """``spfm_explain_topk_csr``: ``(cols, vals)`` of shape (n, K): per row its attributions
        largest by magnitude, by ``|phi|`` descending, then column ascending; rows with fewer
        than K stored entries are padded with column -1 and value 0.  ``K`` above
        ``SPFM_EXPLAIN_MAX_K``: ValueError."""
        K = int(K)
        if K > _capi.EXPLAIN_MAX_K:
            raise ValueError("explain_topk: K = %d exceeds SPFM_EXPLAIN_MAX_K = %d (never answered "
                             "approximately)" % (K, _capi.EXPLAIN_MAX_K))
        Xr, args, keep = self._explain_args(X, blocks, coef, fit_linear, "explain_topk")
        idx = np.full((Xr.shape[0], max(K, 1)), -1, dtype=np.int32)
        val = np.zeros((Xr.shape[0], max(K, 1)))
        self._check(self._lib.spfm_explain_topk_csr(
            *args, K, idx.ctypes.data_as(_capi._ip), val.ctypes.data_as(_capi._dp)))
        return idx, val

    def explain_set_partition(self, slab_nnz=0):
        """``spfm_explain_set_partition``: stored entries per slab of the following explain calls
        (0: the library's default).  No result bit depends on it."""
        self._check(self._lib.spfm_explain_set_partition(self._h, int(slab_nnz)))

    def explain_info(self):
        """``spfm_explain_info``: dict ``scratch_kib`` (device memory the explain calls hold),
        ``device_ms`` (kernels of the last ``explain`` / ``explain_topk``), ``slab_nnz`` as set,
        ``slabs`` of the last call."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._lib.spfm_explain_info(self._h, out.ctypes.data_as(_capi._lp)))
        return dict(scratch_kib=int((out[0] + 1023) // 1024), device_ms=out[1] / 1e3,
                    slab_nnz=int(out[2]), slabs=int(out[3]))

    # ------------------------- per-row pair attributions: values, top-K, group tables (spfm.h)
    def explain_pairs(self, X, blocks, coef, fit_linear, mode="interaction", main=False):
        """``spfm_explain_pairs_csr``: ``(pair_ptr, vals, main)`` for the canonical CSR form of
        ``X``: ``pair_ptr`` (n + 1) the rows' offsets into ``vals``, row ``i`` owning
        ``n_i (n_i - 1) / 2`` values in the order (first position, second position); per pair
        ``phi_iab`` or, with ``mode='hessian'``, ``d2f / dx_ia dx_ib``; ``main`` per stored entry
        (``None`` unless asked for; interaction mode only).  More than ``SPFM_PAIRS_MAX_BYTES`` of
        values: ValueError."""
        if mode not in _capi.PAIRS_MODES:
            raise ValueError("explain_pairs: mode must be 'interaction' or 'hessian', got %r"
                             % (mode,))
        if main and mode != "interaction":
            raise ValueError("explain_pairs: main belongs to mode='interaction'")
        Xr, args, keep = self._explain_args(X, blocks, coef, fit_linear, "explain_pairs")
        n_i = np.diff(Xr.indptr).astype(np.int64)
        ptr = np.concatenate([[0], np.cumsum(n_i * (n_i - 1) // 2)]).astype(np.int64)
        if 8 * int(ptr[-1]) > _capi.PAIRS_MAX_BYTES:
            raise ValueError("explain_pairs: %d pairs to list, more than SPFM_PAIRS_MAX_BYTES = %d "
                             "bytes of values" % (int(ptr[-1]), _capi.PAIRS_MAX_BYTES))
        vals = np.zeros(int(ptr[-1]))
        mn = np.zeros(Xr.nnz) if main else None
        self._check(self._lib.spfm_explain_pairs_csr(
            *args, _capi.PAIRS_MODES[mode], vals.ctypes.data_as(_capi._dp),
            mn.ctypes.data_as(_capi._dp) if main else None))
        return ptr, vals, mn

    def explain_pairs_topk(self, X, blocks, coef, fit_linear, K, mode="interaction"):
        """``spfm_explain_pairs_topk_csr``: ``(col_a, col_b, vals)`` of shape (n, K): per row its
        pairs largest by magnitude, by ``|value|`` descending, then pair index ascending; rows with
        fewer than K pairs are padded with -1, -1 and 0.  ``K`` above ``SPFM_PAIRS_MAX_K``:
        ValueError."""
        K = int(K)
        if mode not in _capi.PAIRS_MODES:
            raise ValueError("explain_pairs_topk: mode must be 'interaction' or 'hessian', got %r"
                             % (mode,))
        if K > _capi.PAIRS_MAX_K:
            raise ValueError("explain_pairs_topk: K = %d exceeds SPFM_PAIRS_MAX_K = %d (never "
                             "answered approximately)" % (K, _capi.PAIRS_MAX_K))
        Xr, args, keep = self._explain_args(X, blocks, coef, fit_linear, "explain_pairs_topk")
        ca = np.full((Xr.shape[0], max(K, 1)), -1, dtype=np.int32)
        cb = np.full((Xr.shape[0], max(K, 1)), -1, dtype=np.int32)
        val = np.zeros((Xr.shape[0], max(K, 1)))
        self._check(self._lib.spfm_explain_pairs_topk_csr(
            *args, _capi.PAIRS_MODES[mode], K, ca.ctypes.data_as(_capi._ip),
            cb.ctypes.data_as(_capi._ip), val.ctypes.data_as(_capi._dp)))
        return ca, cb, val

    def explain_pairs_grouped(self, X, blocks, coef, fit_linear, G, group):
        """``spfm_explain_pairs_grouped_csr``: ``(cells, main)``: (n, G (G + 1) / 2) the upper
        triangles of the rows' group x group tables, cell ``(g, h)``, ``g <= h``, at
        ``g G - g (g - 1) / 2 + h - g``, and (n, G) the main effects summed per group.  ``group``:
        int ids in ``[0, G)``, one per feature.  ``G`` above ``SPFM_PAIRS_MAX_GROUPS``:
        ValueError."""
        G = int(G)
        if G > _capi.PAIRS_MAX_GROUPS:
            raise ValueError("explain_pairs_grouped: G = %d exceeds SPFM_PAIRS_MAX_GROUPS = %d"
                             % (G, _capi.PAIRS_MAX_GROUPS))
        Xr, args, keep = self._explain_args(X, blocks, coef, fit_linear, "explain_pairs_grouped")
        group = np.ascontiguousarray(group, dtype=np.int32)
        if group.shape != (self.d,):
            raise ValueError("explain_pairs_grouped: group must hold one id per feature (%d), got "
                             "shape %r" % (self.d, group.shape))
        ga, gp = _capi.i32(group)
        cells = np.zeros((Xr.shape[0], max(G, 1) * (max(G, 1) + 1) // 2))
        mn = np.zeros((Xr.shape[0], max(G, 1)))
        self._check(self._lib.spfm_explain_pairs_grouped_csr(
            *args, G, gp, cells.ctypes.data_as(_capi._dp), mn.ctypes.data_as(_capi._dp)))
        return cells, mn

    # ------------------------- model banks: F models scored in one pass over the rows (spfm.h)
    def bank_set(self, koff, degrees, Pt_bank, lams_bank, w_bank=None):
        """``spfm_bank_set``: make the stacked image resident.  ``Pt_bank`` (n_blocks, d, S),
        ``lams_bank`` (S), ``w_bank`` (d, F) or ``None`` (no linear term), ``koff`` (F + 1),
        ``degrees`` the blocks' degrees (-1: all-subsets)."""
        Pt_bank = np.ascontiguousarray(Pt_bank, dtype=np.float64)
        if Pt_bank.ndim != 3:
            raise ValueError("bank_set: Pt_bank must be (n_blocks, n_features, S)")
        nb, d, S = Pt_bank.shape
        ka, kp = _capi.i32(koff)
        ga, gp = _capi.i32(degrees)
        la, lp = _capi.f64(lams_bank)
        F = ka.shape[0] - 1
        if ga.shape[0] != nb or la.shape[0] != S or F < 0 or (F >= 1 and ka[-1] != S):
            raise ValueError("bank_set: koff / degrees / lams_bank do not match Pt_bank")
        wp = None
        if w_bank is not None:
            wa, wp = _capi.f64(w_bank)
            if wa.shape != (d, F):
                raise ValueError("bank_set: w_bank must be (n_features, F)")
        self._check(self._lib.spfm_bank_set(self._h, d, F, kp, nb, gp,
                                            Pt_bank.ctypes.data_as(_capi._dp), lp, wp))
        self.bank_shape = (F, S, d)

    def _bank_args(self, X, what):
        """-> (rows, the six leading arguments of the four passes, what keeps them alive)"""
        if getattr(self, "bank_shape", None) is None:
            raise ValueError("%s: call bank_set first" % what)
        Xr = sp.csr_matrix(X, dtype=np.float64)
        if not Xr.has_canonical_format:
            Xr = Xr.copy()
            Xr.sum_duplicates()
            Xr.sort_indices()
        keep = (_capi.i64(Xr.indptr), _capi.i32(Xr.indices), _capi.f64(Xr.data))
        return Xr.shape[0], (self._h, Xr.shape[0], Xr.shape[1], keep[0][1], keep[1][1],
                             keep[2][1]), keep

    def bank_scores(self, X):
        """``spfm_bank_scores``: float64 (n, F), every model's ``decision_function``."""
        n, args, keep = self._bank_args(X, "bank_scores")
        out = np.zeros((n, self.bank_shape[0]))
        self._check(self._lib.spfm_bank_scores(*args, out.ctypes.data_as(_capi._dp)))
        return out

    def bank_argmax(self, X):
        """``spfm_bank_argmax``: ``(index int32, best, runner_up)``, (n,) each; ties go to the
        lowest index, the runner-up of a one-model bank is ``-inf``."""
        n, args, keep = self._bank_args(X, "bank_argmax")
        idx, best, runner = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
        self._check(self._lib.spfm_bank_argmax(
            *args, idx.ctypes.data_as(_capi._ip), best.ctypes.data_as(_capi._dp),
            runner.ctypes.data_as(_capi._dp)))
        return idx, best, runner

    def bank_losses(self, X, y, loss):
        """``spfm_bank_losses``: (F,) sums of ``loss(score_if, y_i)`` (``y`` (n,)) or of
        ``loss(score_if, y_if)`` (``y`` (n, F))."""
        if loss not in _capi.LOSSES:
            raise ValueError("bank_losses: loss must be one of %s, got %r"
                             % (sorted(_capi.LOSSES), loss))
        n, args, keep = self._bank_args(X, "bank_losses")
        ya, yp = _capi.f64(y)
        F = self.bank_shape[0]
        if ya.shape not in ((n,), (n, F)):
            raise ValueError("bank_losses: y must be (%d,) or (%d, %d), got %r"
                             % (n, n, F, ya.shape))
        out = np.zeros(F)
        self._check(self._lib.spfm_bank_losses(*args, _capi.LOSSES[loss], yp, int(ya.ndim == 2),
                                               out.ctypes.data_as(_capi._dp)))
        return out

    def bank_group_sums(self, X, y, weight, group, G, metrics):
        """``spfm_bank_group_sums``: float64 (Q, F, G), cell [q, f, g] the sum over the rows of
        group ``g`` of ``weight_i * metric_q(score_if, y_if)``.  ``y`` (n,) or (n, F); ``weight``
        (n,) float64 or ``None`` (1.0); ``group`` (n,) int32 or ``None`` (all 0); ``metrics`` a
        sequence of names from ``_capi.BANK_METRICS``."""
        for m in metrics:
            if m not in _capi.BANK_METRICS:
                raise ValueError("bank_group_sums: metrics must be among %s, got %r"
                                 % (sorted(_capi.BANK_METRICS), m))
        n, args, keep = self._bank_args(X, "bank_group_sums")
        ya, yp = _capi.f64(y)
        F = self.bank_shape[0]
        if ya.shape not in ((n,), (n, F)):
            raise ValueError("bank_group_sums: y must be (%d,) or (%d, %d), got %r"
                             % (n, n, F, ya.shape))
        wp = gp = None
        if weight is not None:
            wa, wp = _capi.f64(weight)
            if wa.shape != (n,):
                raise ValueError("bank_group_sums: weight must be (%d,), got %r" % (n, wa.shape))
        if group is not None:
            ga, gp = _capi.i32(group)
            if ga.shape != (n,):
                raise ValueError("bank_group_sums: group must be (%d,), got %r" % (n, ga.shape))
        ma, mp = _capi.i32([_capi.BANK_METRICS[m] for m in metrics])
        out = np.zeros((len(metrics), F, max(int(G), 1)))
        self._check(self._lib.spfm_bank_group_sums(*args, yp, int(ya.ndim == 2), wp, gp, int(G),
                                                   len(metrics), mp,
                                                   out.ctypes.data_as(_capi._dp)))
        return out

    def bank_group_auc(self, X, y, weight, group, G, sets):
        """``spfm_bank_group_auc``: ``(out float64 (F, U, 3), pairs int64 (F, U, 3) or None)``:
        per member and set ``auc, pos_weight, neg_weight`` and, unweighted, ``U2, n_pos, n_neg``.
        ``y`` (n,) or (n, F); ``weight`` (n,) float64 or ``None`` (the integer path); ``group`` (n,)
        int32 or ``None`` (all 0); ``sets`` uint32 (F, U) bitmasks over the groups or ``None`` (one
        set per group)."""
        n, args, keep = self._bank_args(X, "bank_group_auc")
        ya, yp = _capi.f64(y)
        F = self.bank_shape[0]
        if ya.shape not in ((n,), (n, F)):
            raise ValueError("bank_group_auc: y must be (%d,) or (%d, %d), got %r"
                             % (n, n, F, ya.shape))
        wp = gp = sp_ = None
        if weight is not None:
            wa, wp = _capi.f64(weight)
            if wa.shape != (n,):
                raise ValueError("bank_group_auc: weight must be (%d,), got %r" % (n, wa.shape))
        if group is not None:
            ga, gp = _capi.i32(group)
            if ga.shape != (n,):
                raise ValueError("bank_group_auc: group must be (%d,), got %r" % (n, ga.shape))
        U = max(int(G), 1)
        if sets is not None:
            sa = np.ascontiguousarray(sets, dtype=np.uint32)
            if sa.ndim != 2 or sa.shape[0] != F:
                raise ValueError("bank_group_auc: sets must be (%d, U), got %r" % (F, sa.shape))
            U, sp_ = sa.shape[1], sa.ctypes.data_as(_capi._up)
        out = np.zeros((F, max(U, 1), 3))
        pairs = np.zeros((F, max(U, 1), 3), dtype=np.int64) if weight is None else None
        self._check(self._lib.spfm_bank_group_auc(
            *args, yp, int(ya.ndim == 2), wp, gp, int(G), sp_, int(U),
            out.ctypes.data_as(_capi._dp),
            None if pairs is None else pairs.ctypes.data_as(_capi._lp)))
        return out, pairs

    def bank_group_curve(self, X, y, weight, group, G, sets, auc=False):
        """``spfm_bank_group_curve``: ``(out float64 (F, U, 11), counts int64 (F, U, 6) or None,
        auc_out float64 (F, U, 3) or None, auc_pairs int64 (F, U, 3) or None)``: per member and set
        ``ap, f1, f1_thr, f1_tp, f1_fp, ks, ks_thr, ks_tp, ks_fp, pos_weight, neg_weight`` and,
        unweighted, ``n_pos, n_neg, f1_tp, f1_fp, ks_tp, ks_fp``; with ``auc`` the tables of
        ``bank_group_auc`` from the same pass and sorts.  The arguments are ``bank_group_auc``'s."""
        n, args, keep = self._bank_args(X, "bank_group_curve")
        ya, yp = _capi.f64(y)
        F = self.bank_shape[0]
        if ya.shape not in ((n,), (n, F)):
            raise ValueError("bank_group_curve: y must be (%d,) or (%d, %d), got %r"
                             % (n, n, F, ya.shape))
        wp = gp = sp_ = None
        if weight is not None:
            wa, wp = _capi.f64(weight)
            if wa.shape != (n,):
                raise ValueError("bank_group_curve: weight must be (%d,), got %r" % (n, wa.shape))
        if group is not None:
            ga, gp = _capi.i32(group)
            if ga.shape != (n,):
                raise ValueError("bank_group_curve: group must be (%d,), got %r" % (n, ga.shape))
        U = max(int(G), 1)
        if sets is not None:
            sa = np.ascontiguousarray(sets, dtype=np.uint32)
            if sa.ndim != 2 or sa.shape[0] != F:
                raise ValueError("bank_group_curve: sets must be (%d, U), got %r" % (F, sa.shape))
            U, sp_ = sa.shape[1], sa.ctypes.data_as(_capi._up)
        U1 = max(U, 1)
        out = np.zeros((F, U1, _capi.BANK_CURVE_VALUES))
        ints = weight is None
        counts = np.zeros((F, U1, _capi.BANK_CURVE_COUNTS), dtype=np.int64) if ints else None
        auc_out = np.zeros((F, U1, 3)) if auc else None
        pairs = np.zeros((F, U1, 3), dtype=np.int64) if auc and ints else None
        self._check(self._lib.spfm_bank_group_curve(
            *args, yp, int(ya.ndim == 2), wp, gp, int(G), sp_, int(U),
            out.ctypes.data_as(_capi._dp),
            None if counts is None else counts.ctypes.data_as(_capi._lp),
            None if auc_out is None else auc_out.ctypes.data_as(_capi._dp),
            None if pairs is None else pairs.ctypes.data_as(_capi._lp)))
        return out, counts, auc_out, pairs

    def bank_mean(self, X, weights=None):
        """``spfm_bank_mean``: (n,) ``sum_f weights[f] score_if``, added in model order;
        ``weights`` ``None``: ``1 / F``."""
        n, args, keep = self._bank_args(X, "bank_mean")
        wp = None
        if weights is not None:
            wa, wp = _capi.f64(weights)
            if wa.shape != (self.bank_shape[0],):
                raise ValueError("bank_mean: weights must be (%d,), got %r"
                                 % (self.bank_shape[0], wa.shape))
        out = np.zeros(n)
        self._check(self._lib.spfm_bank_mean(*args, wp, out.ctypes.data_as(_capi._dp)))
        return out

    def bank_set_partition(self, slab_nnz=0):
        """``spfm_bank_set_partition``: stored entries per slab of the following bank passes
        (0: the library's default).  No bit of a score depends on it."""
        self._check(self._lib.spfm_bank_set_partition(self._h, int(slab_nnz)))

    def bank_info(self):
        """``spfm_bank_info``: dict ``slabs`` and ``launches`` (of ``bank_predict_kernel``) of the
        last pass, ``resident_bytes`` of the image, ``S`` its stacked components."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self._lib.spfm_bank_info(self._h, out.ctypes.data_as(_capi._lp)))
        return dict(slabs=int(out[0]), launches=int(out[1]), resident_bytes=int(out[2]),
                    S=int(out[3]))

    def bank_release(self):
        """``spfm_bank_release``: free the image and the scratch of the bank passes."""
        self._check(self._lib.spfm_bank_release(self._h))
        self.bank_shape = None

    # ------------------------- fold-in of new columns: per-column convex solves (spfm.h)
    def foldin(self, X, y, blocks, coef, fit_linear, offset, loss, cols, alpha, beta, max_iter=50,
               tol=1e-8):
        """``spfm_foldin_csr``: the parameters of the target columns ``cols`` estimated from the
        rows of ``X`` that store them, everything else fixed.  Returns a dict: ``theta``
        (n_cols, R) with ``R = n_blocks k (+ 1)`` (the linear weight first, then the blocks in
        the caller's order), ``n_rows``, ``n_iter``, ``converged``, ``grad_norm``, ``obj0``,
        ``obj1`` per column.  ``blocks`` / ``coef`` as for ``explain``; ``offset``: a constant of
        the model added to every row's output; ``loss`` a key of ``_capi.LOSSES``."""
        if loss not in _capi.LOSSES:
            raise ValueError("foldin: unknown loss %r" % (loss,))
        Xr, args, keep = self._explain_args(X, blocks, coef, fit_linear, "foldin")
        ya, yp = _capi.f64(y)
        if ya.shape != (Xr.shape[0],):
            raise ValueError("foldin: y must hold one target per row")
        ca, cp = _capi.i32(cols)
        m = ca.shape[0]
        R = len(blocks) * self.k + int(bool(fit_linear))
        theta = np.zeros((m, R))
        n_rows = np.zeros(m, dtype=np.int64)
        n_iter = np.zeros(m, dtype=np.int32)
        conv = np.zeros(m, dtype=np.int32)
        gn, o0, o1 = np.zeros(m), np.zeros(m), np.zeros(m)
        dp, ip = _capi._dp, _capi._ip
        self._check(self._lib.spfm_foldin_csr(
            *args[:5], yp, *args[5:], float(offset), _capi.LOSSES[loss], m, cp, float(alpha),
            float(beta), int(max_iter), float(tol), theta.ctypes.data_as(dp),
            n_rows.ctypes.data_as(_capi._lp), n_iter.ctypes.data_as(ip), conv.ctypes.data_as(ip),
            gn.ctypes.data_as(dp), o0.ctypes.data_as(dp), o1.ctypes.data_as(dp)))
        return dict(theta=theta, n_rows=n_rows, n_iter=n_iter, converged=conv.astype(bool),
                    grad_norm=gn, obj0=o0, obj1=o1)

    def foldin_set_partition(self, max_rows=0):
        """``spfm_foldin_set_partition``: rows per group of target columns of the following
        fold-in calls (0: what fits the scratch).  No result bit depends on it."""
        self._check(self._lib.spfm_foldin_set_partition(self._h, int(max_rows)))

    def foldin_info(self):
        """``spfm_foldin_info``: dict ``scratch_kib`` (device memory the fold-in holds),
        ``device_ms`` (kernels of the last call), ``max_rows`` as set, ``groups`` and
        ``ignored_rows`` of the last call."""
        out = np.zeros(5, dtype=np.int64)
        self._check(self._lib.spfm_foldin_info(self._h, out.ctypes.data_as(_capi._lp)))
        return dict(scratch_kib=int((out[0] + 1023) // 1024), device_ms=out[1] / 1e3,
                    max_rows=int(out[2]), groups=int(out[3]), ignored_rows=int(out[4]))

    # ------------------------- third-order weights T[a, j, l] = sum_s lams_s p_sa p_sj p_sl (spfm.h)
    def interaction3_stats(self, order_idx, tol=0.0, n_features=None):
        """``spfm_interaction3_stats``: dict ``nnz`` (triples a < j < l with ``|T| > tol``),
        ``active_features``, ``sum_sq``, ``sum_abs``, ``max_abs`` of the LIVE block
        (``n_features``: of its first features only)."""
        with self._interaction_features(n_features):
            return self._interaction_stats_dict(self._lib.spfm_interaction3_stats, order_idx, tol)

    def interaction3_topk(self, order_idx, K, n_features=None):
        """``spfm_interaction3_topk``: ``(i, j, l, vals)`` of the K largest ``|T|`` among
        ``T != 0`` (``i < j < l``), by ``|T|`` descending, then ``i``, ``j``, ``l``."""
        K = int(K)
        with self._interaction_features(n_features):
            return self._interaction_out(
                lambda *out: self._lib.spfm_interaction3_topk(self._h, int(order_idx), K, *out),
                3, K)

    def interaction3_list(self, order_idx, tol, capacity, n_features=None):
        """``spfm_interaction3_list``: ``(i, j, l, vals)`` of every triple with ``|T| > tol``,
        sorted by ``(i, j, l)``.  ``ValueError`` naming the count when it exceeds ``capacity``."""
        capacity = int(capacity)
        with self._interaction_features(n_features):
            return self._interaction_out(
                lambda *out: self._lib.spfm_interaction3_list(
                    self._h, int(order_idx), float(tol), capacity, *out), 3, capacity)

    def interaction3_values(self, order_idx, i, j, l):
        """``spfm_interaction3_values``: ``T[i[q], j[q], l[q]]``, the three ids in any order (0
        where two of them are equal)."""
        ia, ip = _capi.i32(i)
        ja, jp = _capi.i32(j)
        la, lp = _capi.i32(l)
        if ia.ndim != 1 or ia.shape != ja.shape or ia.shape != la.shape:
            raise ValueError("i, j and l must be 1-d arrays of one length")
        vals = np.zeros(ia.shape[0])
        self._check(self._lib.spfm_interaction3_values(
            self._h, int(order_idx), ia.shape[0], ip, jp, lp, vals.ctypes.data_as(_capi._dp)))
        return vals

    # -------------------------------------------------------------- schedule
    def set_schedule(self, mode, indices_feature, conflict_csc=None):
        """Fix the coordinate order for the next epochs; returns the order used.
        ``conflict_csc``: global CSC structure (multi-GPU) for the disjointness test."""
        jf, jp = _capi.i32(indices_feature)
        order = np.empty(self.d, dtype=np.int32)
        nb = C.c_int32()
        if conflict_csc is None:
            cp, ci, rows = None, None, 0
        else:
            cpa, cp = _capi.i64(conflict_csc.indptr)
            cia, ci = _capi.i32(conflict_csc.indices)
            rows = conflict_csc.shape[0]
        self._check(self._lib.spfm_set_schedule(
            self._h, _capi.SCHEDULES[mode], jp, cp, ci, rows,
            order.ctypes.data_as(_capi._ip), C.byref(nb)))
        self.order, self.n_batches = order, nb.value
        return order

    def get_schedule(self, mode="colored"):
        """The installed schedule as a reusable ``Schedule`` object."""
        from .schedule import Schedule

        nb = C.c_int32()
        self._check(self._lib.spfm_get_schedule(self._h, None, None, C.byref(nb)))
        order = np.empty(self.d, dtype=np.int32)
        bp = np.empty(nb.value + 1, dtype=np.int32)
        self._check(self._lib.spfm_get_schedule(self._h, order.ctypes.data_as(_capi._ip),
                                                bp.ctypes.data_as(_capi._ip), C.byref(nb)))
        return Schedule(order, bp, mode, (self.n, self.d))

    def install_schedule(self, sched, conflict_csc=None):
        """Install a precomputed ``sparsepoly_amd.schedule.Schedule`` (validated by the
        library against the data / the global structure)."""
        oa, op = _capi.i32(sched.order)
        ba, bp = _capi.i32(sched.batch_ptr)
        if oa.shape[0] != self.d:
            raise ValueError("schedule has %d features, the data has %d" % (oa.shape[0], self.d))
        if conflict_csc is None:
            cp, ci, rows = None, None, 0
        else:
            cpa, cp = _capi.i64(conflict_csc.indptr)
            cia, ci = _capi.i32(conflict_csc.indices)
            rows = conflict_csc.shape[0]
        self._check(self._lib.spfm_set_schedule_raw(self._h, op, bp, ba.shape[0] - 1, cp, ci,
                                                    rows))
        self.order, self.n_batches = oa.copy(), ba.shape[0] - 1
        return self.order

    # ---------------------------------------------------------------- epochs
    def cd_linear_epoch(self, alpha):
        v = C.c_double()
        self._check(self._lib.spfm_cd_linear_epoch(self._h, float(alpha), C.byref(v)))
        return v.value

    def pcd_epoch(self, order_idx, degree, beta, gamma, eta, indices_component):
        ic, icp = _capi.i32(indices_component)
        v = C.c_double()
        self._check(self._lib.spfm_pcd_epoch(
            self._h, int(order_idx), int(degree), float(beta), float(gamma), float(eta), icp,
            ic.shape[0], C.byref(v)))
        return v.value

    def pbcd_epoch(self, order_idx, degree, beta, gamma, eta):
        v = C.c_double()
        self._check(self._lib.spfm_pbcd_epoch(
            self._h, int(order_idx), int(degree), float(beta), float(gamma), float(eta),
            C.byref(v)))
        return v.value

    # ---------------------------------------- host-stepped epochs (plug-in regularizers)
    _MU = {"squared": 1.0, "logistic": 0.25, "squared_hinge": 2.0}  # loss.py:18,32,59

    def _host_steps(self):
        sched = self.get_schedule()
        return sched.order, sched.batch_ptr

    def pcd_epoch_host(self, reg, P, lams, loss, order_idx, degree, beta, gamma, eta,
                       indices_component):
        """``pcd.pcd_epoch`` (optimizer/pcd.py:71-137) for a regularizer OBJECT that is not one
        of the device built-ins: the device forms every dependent step's column sums and
        scatter-updates, the object's ``compute_cache_pcd_all / compute_cache_pcd / prox_cd /
        update_cache_pcd`` run here, column by column in visiting order (include/spfm.h
        "host-stepped epochs").  ``P``: the (n_components, n_features) host array of this order,
        updated in place (it mirrors the device copy).  Returns sum_viol."""
        mu = self._MU[loss]
        order, bp = self._host_steps()
        self._check(self._lib.spfm_host_epoch_begin(self._h, int(order_idx), int(degree)))
        reg.compute_cache_pcd_all(P, degree)                                   # pcd.py:91
        viol = 0.0
        sums = np.empty((int(np.diff(bp).max()), 2))
        for s in indices_component:                                            # :92
            s = int(s)
            self._check(self._lib.spfm_host_pass_begin(self._h, s))
            reg.compute_cache_pcd(P, degree, s)                                # :96
            for b in range(len(bp) - 1):
                cols = order[bp[b]:bp[b + 1]]
                nc = len(cols)
                if nc == 0:
                    continue
                self._check(self._lib.spfm_host_step_sums(self._h, b,
                                                          sums.ctypes.data_as(_capi._dp)))
                p_new = np.empty(nc)
                for q in range(nc):                                            # :97, in order
                    j = int(cols[q])
                    p_old = float(P[s, j])
                    inv = mu * sums[q, 1] + beta                               # :61-62
                    upd = (lams[s] * sums[q, 0] + beta * p_old) / inv          # :64-66
                    pn = float(reg.prox_cd(p_old - eta * upd, eta * gamma / inv, degree, j))
                    viol += abs(p_old - pn)                                    # :119-121
                    P[s, j] = pn
                    p_new[q] = pn
                    reg.update_cache_pcd(P, degree, s, j)                      # :135
                self._check(self._lib.spfm_host_step_apply(
                    self._h, b, p_new.ctypes.data_as(_capi._dp), None))
        dv = C.c_double()
        self._check(self._lib.spfm_host_epoch_end(self._h, C.byref(dv)))
        return viol

    def pbcd_epoch_host(self, reg, Pt, lams, loss, order_idx, degree, beta, gamma, eta):
        """``pbcd.pbcd_epoch`` (optimizer/pbcd.py:82-148) for a regularizer object:
        ``compute_cache_pbcd / prox_bcd (in place) / update_cache_pbcd`` run here.  ``Pt``: the
        (n_features, n_components) host array of this order, updated in place."""
        mu = self._MU[loss]
        order, bp = self._host_steps()
        k = Pt.shape[1]
        lams = np.asarray(lams, dtype=np.float64)
        self._check(self._lib.spfm_host_epoch_begin(self._h, int(order_idx), int(degree)))
        reg.compute_cache_pbcd(Pt, degree)                                     # pbcd.py:109
        viol = 0.0
        sums = np.empty((int(np.diff(bp).max()), k + 1))
        for b in range(len(bp) - 1):
            cols = order[bp[b]:bp[b + 1]]
            nc = len(cols)
            if nc == 0:
                continue
            self._check(self._lib.spfm_host_step_sums(self._h, b, sums.ctypes.data_as(_capi._dp)))
            p_new = np.empty((nc, k))
            p_old = np.empty((nc, k))
            for q in range(nc):                                                # :110, in order
                j = int(cols[q])
                p_old[q] = Pt[j]
                inv = mu * sums[q, k] + beta                                   # :68-72
                grad = (sums[q, :k] * lams + beta * Pt[j]) / inv               # :74-77
                pj = Pt[j] - eta * grad                                        # :78
                reg.prox_bcd(pj, eta * gamma / inv, degree, j)                 # :79 (in place)
                viol += float(np.abs(p_old[q] - pj).sum())                     # :146
                Pt[j] = pj
                p_new[q] = pj
                reg.update_cache_pbcd(Pt, degree, j)                           # :145
            self._check(self._lib.spfm_host_step_apply(
                self._h, b, p_new.ctypes.data_as(_capi._dp), p_old.ctypes.data_as(_capi._dp)))
        dv = C.c_double()
        self._check(self._lib.spfm_host_epoch_end(self._h, C.byref(dv)))
        return viol

    def psgd_epoch(self, degree, alpha, beta, gamma, eta0, learning_rate, power_t, batch_size,
                   indices_samples, fit_linear, it, row_lo=None):
        """``psgd.psgd_epoch`` (optimizer/psgd.py:125-199).  Returns (sum_loss, it).
        ``row_lo`` (several ranks, ``spfm_psgd_epoch_sharded``): the handle holds the rows from
        ``row_lo`` on of the problem whose GLOBAL visiting order ``indices_samples`` is; the
        minibatch gradients are all-reduced, ``sum_loss`` is the global sum."""
        idx = np.ascontiguousarray(indices_samples, dtype=np.int32)
        itc = C.c_int64(int(it))
        sl = C.c_double()
        lr = (_capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str)
              else int(learning_rate))
        if row_lo is not None:
            self._check(self._lib.spfm_psgd_epoch_sharded(
                self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
                float(power_t), int(batch_size), idx.ctypes.data_as(_capi._ip), idx.size,
                int(row_lo), int(bool(fit_linear)), C.byref(itc), C.byref(sl)))
            return sl.value, itc.value
        self._check(self._lib.spfm_psgd_epoch(
            self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
            float(power_t), int(batch_size), idx.ctypes.data_as(_capi._ip), idx.size,
            int(bool(fit_linear)), C.byref(itc), C.byref(sl)))
        return sl.value, itc.value

    def psgd_set_adaptive(self, mode, initial_accumulator=1.0, acc_P=None, acc_w=None):
        """Per-feature AdaGrad steps for every psgd / pairs / lists epoch of this handle
        (``spfm_psgd_set_adaptive``).  ``mode``: 0 off, 1 (or
        ``'adagrad'``) on; ``acc_P`` (n_orders, d) / ``acc_w`` (d): accumulators to start from,
        ``None``: zeros.  The epoch calls' ``learning_rate`` then gives the base rate."""
        mode = 1 if mode == "adagrad" else int(mode)
        Pp = wp = None
        if acc_P is not None:
            Pa, Pp = _capi.f64(acc_P)
            if Pa.size != self.n_orders * self.d:
                raise ValueError("acc_P must hold n_orders * d values")
        if acc_w is not None:
            wa, wp = _capi.f64(acc_w)
            if wa.size != self.d:
                raise ValueError("acc_w must hold d values")
        self._check(self._lib.spfm_psgd_set_adaptive(self._h, mode, float(initial_accumulator),
                                                     Pp, wp))

    def psgd_get_adaptive(self):
        """``(A_P (n_orders, d), A_w (d,))``: the accumulators of the adaptive steps as they
        stand (``spfm_psgd_get_adaptive``)."""
        aP = np.empty((self.n_orders, self.d))
        aw = np.empty(self.d)
        self._check(self._lib.spfm_psgd_get_adaptive(
            self._h, aP.ctypes.data_as(_capi._dp), aw.ctypes.data_as(_capi._dp)))
        return aP, aw

    @staticmethod
    def _triples(triples):
        t = np.ascontiguousarray(triples, dtype=np.int32)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("triples must have shape (m, 3), got %r" % (t.shape,))
        return t

    def psgd_pairs_epoch(self, degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                         batch_size, triples, fit_linear, it):
        """One pass of minibatch psgd over the triples (anchor, plus, minus) -- rows of the
        handle's data ``[X; Z]`` -- in the order given (``spfm_psgd_pairs_epoch``).  Returns
        (sum_loss, it)."""
        t = self._triples(triples)
        itc = C.c_int64(int(it))
        sl = C.c_double()
        lr = (_capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str)
              else int(learning_rate))
        self._check(self._lib.spfm_psgd_pairs_epoch(
            self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
            float(power_t), int(batch_size), t.ctypes.data_as(_capi._ip), t.shape[0],
            int(bool(fit_linear)), C.byref(itc), C.byref(sl)))
        return sl.value, itc.value

    def psgd_pairs_epoch_weighted(self, degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                  batch_size, triples, weights, fit_linear, it):
        """``psgd_pairs_epoch`` with one weight ``>= 0`` per triple, which multiplies its loss
        and its gradient (``spfm_psgd_pairs_epoch_weighted``).  Returns
        (sum of weight * loss, it)."""
        t = self._triples(triples)
        wt = np.ascontiguousarray(weights, dtype=np.float64)
        if wt.shape != (t.shape[0],):
            raise ValueError("weights must have shape (%d,), got %r" % (t.shape[0], wt.shape))
        itc = C.c_int64(int(it))
        sl = C.c_double()
        lr = (_capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str)
              else int(learning_rate))
        self._check(self._lib.spfm_psgd_pairs_epoch_weighted(
            self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
            float(power_t), int(batch_size), t.ctypes.data_as(_capi._ip),
            wt.ctypes.data_as(_capi._dp), t.shape[0], int(bool(fit_linear)), C.byref(itc),
            C.byref(sl)))
        return sl.value, itc.value

    def psgd_pairs_eval(self, degree, fit_linear, triples):
        """(sum of the triples' losses, number of triples with margin > 0) at the live device
        parameters; nothing is updated (``spfm_psgd_pairs_eval``)."""
        t = self._triples(triples)
        sl = C.c_double()
        no = C.c_int64()
        self._check(self._lib.spfm_psgd_pairs_eval(
            self._h, int(degree), int(bool(fit_linear)), t.ctypes.data_as(_capi._ip), t.shape[0],
            C.byref(sl), C.byref(no)))
        return sl.value, no.value

    def psgd_pairs_set_sampler(self, n_ctx, n_cand, positives, forbidden=None):
        """Hand the positives -- a sparse ``(n_ctx, n_cand)`` matrix, pattern only -- and the
        forbidden set (the same shape, a superset; ``None``: the positives) to the device sampler
        of the pairwise fit (``spfm_psgd_pairs_set_sampler``).  Rows ``[0, n_ctx)`` of the
        handle's data are the contexts, the next ``n_cand`` the candidates."""
        def csr(M):
            M = sp.csr_matrix(M)
            if not M.has_sorted_indices:
                M = M.sorted_indices()
            return (np.ascontiguousarray(M.indptr, dtype=np.int64),
                    np.ascontiguousarray(M.indices, dtype=np.int32))

        pp, pi = csr(positives)
        if forbidden is None:
            fp = fi = None
        else:
            fp, fi = csr(forbidden)
        self._check(self._lib.spfm_psgd_pairs_set_sampler(
            self._h, int(n_ctx), int(n_cand), pp.ctypes.data_as(_capi._lp),
            pi.ctypes.data_as(_capi._ip),
            None if fp is None else fp.ctypes.data_as(_capi._lp),
            None if fi is None else fi.ctypes.data_as(_capi._ip)))
        self._sampler_npos = int(pp[-1])

    def psgd_pairs_sample(self, degree, n_negatives, n_candidates, max_draws, seed, epoch,
                          order=None, want_triples=True, want_scores=True):
        """Draw the negatives of every positive on the device at the live parameters and leave
        the triple list resident (``spfm_psgd_pairs_sample``).  Returns ``(m, triples, scores)``:
        the number of triples and the host copies -- ``(m, 3)`` int32 rows of ``[X; Z]`` and
        ``(m,)`` float64, by slot -- or ``None`` for a copy that was not asked for."""
        m = getattr(self, "_sampler_npos", 0) * max(int(n_negatives), 0)
        o = None
        if order is not None:
            o = np.ascontiguousarray(order, dtype=np.int32)
            if o.shape != (m,):
                raise ValueError("order must have shape (%d,), got %r" % (m, o.shape))
        t = np.empty((m, 3), dtype=np.int32) if want_triples else None
        sc = np.empty(m, dtype=np.float64) if want_scores else None
        self._check(self._lib.spfm_psgd_pairs_sample(
            self._h, int(degree), int(n_negatives), int(n_candidates), int(max_draws), int(seed),
            int(epoch), None if o is None else o.ctypes.data_as(_capi._ip),
            None if t is None else t.ctypes.data_as(_capi._ip),
            None if sc is None else sc.ctypes.data_as(_capi._dp)))
        return m, t, sc

    def psgd_pairs_set_proposal(self, cum):
        """The proposal distribution of the device samplers: ``cum`` (n_cand,) uint32, the
        inclusive cumulative sums of integer weights (``pairwise.quantise_proposal``), or ``None``
        for the uniform draw (``spfm_psgd_pairs_set_proposal``)."""
        if cum is None:
            self._check(self._lib.spfm_psgd_pairs_set_proposal(self._h, None, 0))
            return
        c = np.ascontiguousarray(cum, dtype=np.uint32)
        self._check(self._lib.spfm_psgd_pairs_set_proposal(
            self._h, c.ctypes.data_as(_capi._up), c.size))

    def psgd_pairs_set_positive_weights(self, weights):
        """One weight ``>= 0`` per positive of the sampler, canonical CSR order, or ``None`` to
        clear (``spfm_psgd_pairs_set_positive_weights``)."""
        if weights is None:
            self._check(self._lib.spfm_psgd_pairs_set_positive_weights(self._h, None, 0))
            return
        wq = np.ascontiguousarray(weights, dtype=np.float64)
        self._check(self._lib.spfm_psgd_pairs_set_positive_weights(
            self._h, wq.ctypes.data_as(_capi._dp), wq.size))

    def psgd_pairs_sample_warp(self, degree, n_negatives, max_trials, max_draws, margin, seed,
                               epoch, order=None, want=True):
        """WARP negatives at the live parameters, left resident with their weights
        (``spfm_psgd_pairs_sample_warp``).  Returns
        ``(m, triples, scores, weights, trials)`` by slot; the four copies are ``None`` without
        ``want``."""
        m = getattr(self, "_sampler_npos", 0) * max(int(n_negatives), 0)
        o = None
        if order is not None:
            o = np.ascontiguousarray(order, dtype=np.int32)
            if o.shape != (m,):
                raise ValueError("order must have shape (%d,), got %r" % (m, o.shape))
        t = np.empty((m, 3), dtype=np.int32) if want else None
        sc = np.empty(m, dtype=np.float64) if want else None
        wt = np.empty(m, dtype=np.float64) if want else None
        tr = np.empty(m, dtype=np.int32) if want else None
        self._check(self._lib.spfm_psgd_pairs_sample_warp(
            self._h, int(degree), int(n_negatives), int(max_trials), int(max_draws),
            float(margin), int(seed), int(epoch),
            None if o is None else o.ctypes.data_as(_capi._ip),
            None if t is None else t.ctypes.data_as(_capi._ip),
            None if sc is None else sc.ctypes.data_as(_capi._dp),
            None if wt is None else wt.ctypes.data_as(_capi._dp),
            None if tr is None else tr.ctypes.data_as(_capi._ip)))
        return m, t, sc, wt, tr

    def psgd_pairs_epoch_sampled(self, degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                 batch_size, fit_linear, it):
        """``psgd_pairs_epoch`` over the list ``psgd_pairs_sample`` left on the device
        (``spfm_psgd_pairs_epoch_sampled``).  Returns (sum_loss, it)."""
        itc = C.c_int64(int(it))
        sl = C.c_double()
        lr = (_capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str)
              else int(learning_rate))
        self._check(self._lib.spfm_psgd_pairs_epoch_sampled(
            self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
            float(power_t), int(batch_size), int(bool(fit_linear)), C.byref(itc), C.byref(sl)))
        return sl.value, itc.value

    @staticmethod
    def _list_loss(list_loss):
        if isinstance(list_loss, str):
            if list_loss not in _capi.LIST_LOSSES:
                raise ValueError("list_loss %r is not supported. Choose from %s."
                                 % (list_loss, sorted(_capi.LIST_LOSSES)))
            return _capi.LIST_LOSSES[list_loss]
        return int(list_loss)

    def psgd_lists_epoch(self, degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                         batch_size, triples, n_negatives, list_loss, fit_linear, it):
        """One pass of minibatch psgd over lists -- a positive with its ``n_negatives``
        negatives, rows ``q M .. q M + M - 1`` of the grouped ``triples`` (rows of ``[X; Z]``) --
        in the order given; ``list_loss``: ``'softmax'`` or ``'list'``; ``batch_size`` counts
        lists (``spfm_psgd_lists_epoch``).  Returns (sum_loss over the lists, it)."""
        t = self._triples(triples)
        itc = C.c_int64(int(it))
        sl = C.c_double()
        lr = (_capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str)
              else int(learning_rate))
        self._check(self._lib.spfm_psgd_lists_epoch(
            self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
            float(power_t), int(batch_size), t.ctypes.data_as(_capi._ip), t.shape[0],
            int(n_negatives), self._list_loss(list_loss), int(bool(fit_linear)), C.byref(itc),
            C.byref(sl)))
        return sl.value, itc.value

    def psgd_lists_epoch_sampled(self, degree, alpha, beta, gamma, eta0, learning_rate, power_t,
                                 batch_size, n_negatives, list_loss, fit_linear, it,
                                 list_order=None):
        """``psgd_lists_epoch`` over the list ``psgd_pairs_sample(order=None)`` left on the
        device; ``list_order``: the visiting order of the lists, or ``None``
        (``spfm_psgd_lists_epoch_sampled``).  Returns (sum_loss, it)."""
        itc = C.c_int64(int(it))
        sl = C.c_double()
        lr = (_capi.LEARNING_RATE[learning_rate] if isinstance(learning_rate, str)
              else int(learning_rate))
        o = None
        if list_order is not None:
            o = np.ascontiguousarray(list_order, dtype=np.int32)
            q = getattr(self, "_sampler_npos", 0)
            if o.shape != (q,):
                raise ValueError("list_order must have shape (%d,), got %r" % (q, o.shape))
        self._check(self._lib.spfm_psgd_lists_epoch_sampled(
            self._h, int(degree), float(alpha), float(beta), float(gamma), float(eta0), lr,
            float(power_t), int(batch_size), int(n_negatives), self._list_loss(list_loss),
            None if o is None else o.ctypes.data_as(_capi._ip), int(bool(fit_linear)),
            C.byref(itc), C.byref(sl)))
        return sl.value, itc.value

    def psgd_lists_eval(self, degree, fit_linear, triples, n_negatives, list_loss):
        """(sum of the lists' losses, number of lists whose positive scores above all of its
        negatives) at the live device parameters; nothing is updated
        (``spfm_psgd_lists_eval``)."""
        t = self._triples(triples)
        sl = C.c_double()
        nf = C.c_int64()
        self._check(self._lib.spfm_psgd_lists_eval(
            self._h, int(degree), int(bool(fit_linear)), t.ctypes.data_as(_capi._ip), t.shape[0],
            int(n_negatives), self._list_loss(list_loss), C.byref(sl), C.byref(nf)))
        return sl.value, nf.value

    # ------------------------------------------------------------- multi-GPU
    @staticmethod
    def comm_unique_id():
        lib = _capi.load()
        buf = C.create_string_buffer(128)
        rc = lib.spfm_comm_unique_id(buf)
        if rc != 0:
            raise SpfmError("spfm_comm_unique_id: %s" % lib.spfm_last_error(None).decode())
        return buf.raw

    def comm_init(self, uid, n_ranks, rank):
        assert len(uid) == 128
        self._check(self._lib.spfm_comm_init(self._h, uid, int(n_ranks), int(rank)))

    def comm_init_shm(self, name, n_ranks, rank):
        """Host shared-memory communicator for ranks sharing one GPU (test / bring-up)."""
        self._check(self._lib.spfm_comm_init_shm(self._h, name.encode(), int(n_ranks), int(rank)))

    def peer_alloc(self):
        """This rank's exchange slab for the in-kernel cross-GPU exchange: its 64-byte IPC
        handle (ship it to every rank, then call ``peer_connect``)."""
        buf = C.create_string_buffer(64)
        self._check(self._lib.spfm_peer_alloc(self._h, buf))
        return buf.raw

    def peer_connect(self, n_ranks, rank, handles):
        """Map the peers' exchange slabs (``handles``: list of n_ranks 64-byte handles in rank
        order).  The persistent passes then run with several ranks; set the schedule after."""
        blob = b"".join(handles)
        assert len(blob) == 64 * n_ranks
        self._check(self._lib.spfm_peer_connect(self._h, int(n_ranks), int(rank), blob))

    # -------------------------------------------------------- instrumentation
    def profile_enable(self, on=True):
        self._check(self._lib.spfm_profile_enable(self._h, int(bool(on))))

    def profile_reset(self):
        self._check(self._lib.spfm_profile_reset(self._h))

    def profile_get(self, which):
        ms, nl, nz = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self._lib.spfm_profile_get(self._h, int(which), C.byref(ms), C.byref(nl),
                                               C.byref(nz)))
        return ms.value, nl.value, nz.value

    def set_use_graph(self, on):
        self._check(self._lib.spfm_set_use_graph(self._h, int(bool(on))))

    def debug_hop_latency(self, partner=1, rounds=20000):
        """(ns per hand-off, (xcc of workgroup 0, xcc of the partner)); see spfm.h."""
        ns = C.c_double()
        xcc = (C.c_int32 * 2)()
        self._check(self._lib.spfm_debug_hop_latency(self._h, int(partner), int(rounds),
                                                     C.byref(ns), xcc))
        return ns.value, (xcc[0], xcc[1])

    def debug_exchange_cost(self, groups=64, ncols=37, readers_mod=1, rounds=5000):
        """ns per bare exchange round of the persistent pass; see spfm.h."""
        ns = C.c_double()
        self._check(self._lib.spfm_debug_exchange_cost(self._h, int(groups), int(ncols),
                                                       int(readers_mod), int(rounds),
                                                       C.byref(ns)))
        return ns.value

    def debug_sweep_sums(self, vals, ncols=64, step=0):
        """Totals of one step's granule sweep over vals[groups, 64, nv] (nv = 1 or 2), as the
        persistent passes form them: array [64, nv]; see spfm.h."""
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert vals.ndim == 3 and vals.shape[1] == 64, vals.shape
        groups, _, nv = vals.shape
        out = np.zeros((64, nv), dtype=np.float64)
        self._check(self._lib.spfm_debug_sweep_sums(
            self._h, int(groups), int(ncols), int(nv), int(step),
            vals.ctypes.data_as(_capi._dp), out.ctypes.data_as(_capi._dp)))
        return out

    def debug_prb_stamps(self):
        buf = np.zeros(16 * 512, dtype=np.int64)
        nv = self._lib.spfm_debug_prb_stamps(self._h, buf.ctypes.data_as(_capi._lp), buf.size)
        if nv < 0:
            self._check(nv)
        return buf[:nv].reshape(-1, 16)

    def debug_branch_counts(self, reset=True):
        """How often the device chains took the reference's "numerical error" branches since
        the last reset: dict with keys omegati_clip (omegati.py:97-98), omegacs_dcache
        (omegacs.py:90-96), omegacs_cache (omegacs.py:75-76), squaredl21_resum
        (squaredl21.py:48-49)."""
        buf = (C.c_uint32 * 8)()
        self._check(self._lib.spfm_debug_branch_counts(self._h, buf, int(bool(reset))))
        return dict(omegati_clip=buf[0], omegacs_dcache=buf[1], omegacs_cache=buf[2],
                    squaredl21_resum=buf[3], relax_steps=buf[4], relax_rounds=buf[5])

    def debug_stream_probe(self):
        """One launch that reads the persistent pass's entry stream and nothing else; returns
        the bytes it requested (counter calibration, see spfm.h)."""
        nb = C.c_int64()
        self._check(self._lib.spfm_debug_stream_probe(self._h, C.byref(nb)))
        return nb.value

    def debug_write_probe(self, bytes_per_record):
        """One launch that stores one record of 4, 8 or 16 bytes per matrix entry at the entry's
        row and writes nothing else; returns the bytes it requested (WRITE_SIZE calibration)."""
        nb = C.c_int64()
        self._check(self._lib.spfm_debug_write_probe(self._h, int(bytes_per_record), C.byref(nb)))
        return nb.value

    def debug_stream_info(self, kind):
        """Shape of the entry stream of ``kind`` ('rowblock', 'relaxed', 'pbcd', 'wide') that the
        handle holds; ValueError if no epoch has built it yet.  See spfm.h."""
        info = np.zeros(8, dtype=np.int64)
        self._check(self._lib.spfm_debug_stream_info(self._h, _capi.STREAMS[kind],
                                                     info.ctypes.data_as(_capi._lp)))
        names = ("G", "nb", "NG", "long_thresh", "balance", "n_entries", "has_long", "device")
        return dict(zip(names, (int(v) for v in info)))

    def debug_stream_tables(self, kind):
        """The tables of that stream, copied out of device memory: the dict of ``stream_build``
        plus ``info``, ``batch_ptr`` (the steps the stream was built for) and, for 'relaxed',
        ``skip``.  Needs the option ``debug_setup_any_size`` = 1 (set before the schedule)."""
        info = self.debug_stream_info(kind)
        nnz = self.nnz  # (the relaxed runs leave entries out: n_entries may be less)
        t = _stream_arrays(kind, self.d, nnz, info["G"], info["nb"], info["NG"])
        bp = np.zeros(info["nb"] + 1, dtype=np.int32)
        skip = np.zeros(nnz, dtype=np.uint8) if kind == "relaxed" else None
        self._check(self._lib.spfm_debug_stream_tables(
            self._h, _capi.STREAMS[kind],
            *(_stream_ptrs(t) + (None if skip is None else skip.ctypes.data_as(_capi._bp),
                                 bp.ctypes.data_as(_capi._ip)))))
        for name in ("src", "flags"):
            if name in t:
                t[name] = t[name][:info["n_entries"]]
        t.update(info=info, batch_ptr=bp, n_entries=info["n_entries"])
        if skip is not None:
            t["skip"] = skip
        return t

    def get_option(self, key):
        v = C.c_int()
        self._check(self._lib.spfm_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def set_option(self, key, value):
        self._check(self._lib.spfm_set_option(self._h, key.encode(), int(value)))
