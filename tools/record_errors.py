"""Drive one handle per storage type through a fixed table of refused calls and write
``(return code, spfm_last_error)`` per case to JSON.

    python tools/record_errors.py profiles/errors_parent_<sha>.json

The table covers every argument check (FAIL or bare SPFM_ERR_INVALID) that inputs of n = 8, d = 5,
k = 2 can reach in spfm_set_data_csr, spfm_set_data_csc, spfm_set_eval_csr, spfm_eval_loss,
spfm_objective_terms, the five spfm_interaction_* entries, the two spfm_gram_* entries and
spfm_predict_csr.  (Not reachable at this size: the tie bound of interaction_topk, which needs
more than 2^20 candidates, and the internal consistency checks that answer SPFM_ERR_RUNTIME.)
tests/test_hip_errors.py replays the table against the recording of the parent commit.

    python tools/record_errors.py --psgd profiles/errors_psgd_parent_<sha>.json

records the second table, the psgd unit's own (PSGD_CASES below), in the same form.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sparsepoly_amd import _capi  # noqa: E402

N, D, K = 8, 5, 2
NULL = None


def _problem():
    rng = np.random.RandomState(7)
    dense = rng.randn(N, D) * (rng.rand(N, D) < 0.6)
    dense[3] = 0.0  # an empty row
    indptr = np.zeros(N + 1, np.int64)
    indices, data = [], []
    for i in range(N):
        nzc = np.flatnonzero(dense[i])
        indices += list(nzc)
        data += list(dense[i, nzc])
        indptr[i + 1] = len(indices)
    return (indptr, np.asarray(indices, np.int32), np.asarray(data, np.float64),
            rng.randn(N), rng.randn(2, K, D), rng.randn(D), np.array([1.0, -1.0]))


INDPTR, INDICES, DATA, Y, P, W, LAMS = _problem()
NNZ = int(INDPTR[-1])


def _csc():
    order = np.lexsort((np.repeat(np.arange(N), np.diff(INDPTR)), INDICES))
    cp = np.zeros(D + 1, np.int64)
    np.add.at(cp, INDICES + 1, 1)
    rows = np.repeat(np.arange(N), np.diff(INDPTR)).astype(np.int32)
    return np.cumsum(cp), rows[order], DATA[order]


CPTR, CROWS, CDATA = _csc()


def ptr(a):
    """ctypes pointer of a numpy array (kept alive by the caller's reference); None -> NULL"""
    if a is None:
        return None
    kind = {np.dtype(np.int64): C.c_int64, np.dtype(np.int32): C.c_int32,
            np.dtype(np.float64): C.c_double}[a.dtype]
    return a.ctypes.data_as(C.POINTER(kind))


def i64(*v):
    return np.asarray(v, np.int64)


def i32(*v):
    return np.asarray(v, np.int32)


def f64(*v):
    return np.asarray(v, np.float64)


class Handle:
    """A fresh handle brought to one of the named states by calls that all succeed."""

    def __init__(self, lib, dtype, state):
        self.lib = lib
        self.h = C.c_void_p()
        assert lib.spfm_create(C.byref(self.h), 0, _capi.DTYPES[dtype]) == 0
        steps = {
            "fresh": "", "data": "d", "params": "p", "model": "dp", "fit": "dpc",
            "eval_no_y": "dpce", "eval_unconfigured": "dpE", "host_ingest": "o",
        }[state]
        for s in steps:
            getattr(self, "_" + s)()

    def ok(self, rc):
        assert rc == 0, (rc, self.lib.spfm_last_error(self.h))

    def _o(self):
        self.ok(self.lib.spfm_set_option(self.h, b"ingest_device", 0))

    def _d(self):
        self.ok(self.lib.spfm_set_data_csr(self.h, N, D, ptr(INDPTR), ptr(INDICES), ptr(DATA), ptr(Y)))

    def _p(self):
        self.ok(self.lib.spfm_set_params(self.h, 2, K, D, ptr(P), ptr(W), ptr(LAMS)))

    def _c(self):
        self.ok(self.lib.spfm_configure(self.h, _capi.SOLVERS["pcd"], _capi.LOSSES["squared"],
                                        _capi.REGULARIZERS["l1"], 2))

    def _e(self):
        self.ok(self.lib.spfm_set_eval_csr(self.h, N, D, ptr(INDPTR), ptr(INDICES), ptr(DATA), NULL))

    def _E(self):
        self.ok(self.lib.spfm_set_eval_csr(self.h, N, D, ptr(INDPTR), ptr(INDICES), ptr(DATA), ptr(Y)))

    def close(self):
        self.lib.spfm_destroy(self.h)


def _cases():
    """(name, state, call(lib, h) -> rc).  `h` is None for the NULL-handle cases."""
    out8, dbl, n_out = np.zeros(8), np.zeros(64), np.zeros(1, np.int64)
    r32, c32, cnt2 = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(2, np.int64)
    big = 1 << 31
    bad_ptr0, not_mono = INDPTR.copy(), INDPTR.copy()
    bad_ptr0[0] = 1
    not_mono[2] = not_mono[3] + 1
    col_hi, col_lo, unsorted, dup = (INDICES.copy() for _ in range(4))
    col_hi[0], col_lo[0] = D, -1
    row0 = slice(int(INDPTR[0]), int(INDPTR[1]))
    assert INDPTR[1] - INDPTR[0] >= 2
    unsorted[row0] = unsorted[row0][::-1]
    dup[1] = dup[0]
    cases = []

    def add(name, state, call):
        cases.append((name, state, call))

    # ---- spfm_set_data_csr / spfm_set_data_csc
    for ent, fn, ip, ix, dat in (("set_data_csr", "spfm_set_data_csr", INDPTR, INDICES, DATA),
                                 ("set_data_csc", "spfm_set_data_csc", CPTR, CROWS, CDATA)):
        def sd(n=N, d=D, indptr=ip, indices=ix, data=dat, y=Y, fn=fn):
            return lambda L, h: getattr(L, fn)(h, n, d, ptr(indptr), ptr(indices), ptr(data), ptr(y))
        bp0, nm = ip.copy(), ip.copy()
        bp0[0] = 1
        nm[2] = nm[3] + 1
        add(ent + ":null_handle", None, sd())
        add(ent + ":n_negative", "fresh", sd(n=-1))
        add(ent + ":d_zero", "fresh", sd(d=0))
        add(ent + ":indptr_null", "fresh", sd(indptr=None))
        add(ent + ":y_null", "fresh", sd(y=None))
        add(ent + ":n_2^31", "fresh", sd(n=big))
        add(ent + ":indptr0", "fresh", sd(indptr=bp0))
        add(ent + ":indptr_not_monotone", "fresh", sd(indptr=nm))
    for state in ("fresh", "host_ingest"):
        for nm_, ix in (("col_high", col_hi), ("col_negative", col_lo), ("unsorted", unsorted),
                        ("duplicate", dup)):
            add("set_data_csr:%s:%s" % (nm_, state), state,
                lambda L, h, ix=ix: L.spfm_set_data_csr(h, N, D, ptr(INDPTR), ptr(ix), ptr(DATA), ptr(Y)))
    rows_hi, rows_lo, rows_uns, rows_dup = (CROWS.copy() for _ in range(4))
    rows_hi[0], rows_lo[0] = N, -1
    c0 = int(np.flatnonzero(np.diff(CPTR) >= 2)[0])
    a = int(CPTR[c0])
    rows_uns[a], rows_uns[a + 1] = CROWS[a + 1], CROWS[a]
    rows_dup[a + 1] = rows_dup[a]
    for nm_, ix in (("row_high", rows_hi), ("row_negative", rows_lo), ("unsorted", rows_uns),
                    ("duplicate", rows_dup)):
        add("set_data_csc:" + nm_, "fresh",
            lambda L, h, ix=ix: L.spfm_set_data_csc(h, N, D, ptr(CPTR), ptr(ix), ptr(CDATA), ptr(Y)))

    # ---- spfm_set_eval_csr
    def se(n=N, d=D, indptr=INDPTR, indices=INDICES, data=DATA, y=Y):
        return lambda L, h: L.spfm_set_eval_csr(h, n, d, ptr(indptr), ptr(indices), ptr(data), ptr(y))
    add("set_eval:null_handle", None, se())
    add("set_eval:rows_negative", "model", se(n=-1))
    add("set_eval:d_zero", "model", se(d=0))
    add("set_eval:indptr_null", "model", se(indptr=None))
    add("set_eval:no_model", "fresh", se())
    add("set_eval:d_differs", "model", se(d=D + 1))
    add("set_eval:d_differs_params_only", "params", se(d=D + 1))
    add("set_eval:rows_2^31", "model", se(n=big))
    add("set_eval:indptr0", "model", se(indptr=bad_ptr0))
    add("set_eval:indptr_not_monotone", "model", se(indptr=not_mono))
    add("set_eval:indices_null", "model", se(indices=None))
    add("set_eval:data_null", "model", se(data=None))
    add("set_eval:col_high", "model", se(indices=col_hi))
    add("set_eval:col_negative", "model", se(indices=col_lo))
    add("set_eval:unsorted", "model", se(indices=unsorted))
    add("set_eval:duplicate", "model", se(indices=dup))

    # ---- spfm_eval_loss
    def el(degree=2, loss=True, pred=True):
        return lambda L, h: L.spfm_eval_loss(h, degree, 1, 0, ptr(dbl) if loss else NULL,
                                             ptr(dbl[8:]) if pred else NULL)
    add("eval_loss:null_handle", None, el())
    add("eval_loss:no_params", "data", el())
    add("eval_loss:no_eval", "fit", el())
    add("eval_loss:degree_0", "eval_no_y", el(degree=0, loss=False))
    add("eval_loss:degree_7", "eval_no_y", el(degree=7, loss=False))
    add("eval_loss:no_targets", "eval_no_y", el())
    add("eval_loss:not_configured", "eval_unconfigured", el())

    # ---- spfm_objective_terms
    def ot(order=0, degree=2, out=out8):
        return lambda L, h: L.spfm_objective_terms(h, order, degree, ptr(out))
    add("objective_terms:null_handle", None, ot())
    add("objective_terms:out_null", "fit", ot(out=None))
    add("objective_terms:no_params", "data", ot())
    add("objective_terms:not_configured", "model", ot())
    add("objective_terms:degree_0", "fit", ot(degree=0))
    add("objective_terms:degree_7", "fit", ot(degree=7))
    add("objective_terms:order_low", "fit", ot(order=-2))
    add("objective_terms:order_high", "fit", ot(order=2))

    # ---- spfm_interaction_*
    nan = float("nan")
    ent = {
        "stats": lambda o=0, tol=0.0, c=cnt2, s=dbl: (
            lambda L, h: L.spfm_interaction_stats(h, o, tol, ptr(c), ptr(s))),
        "topk": lambda o=0, k=3, r=r32, c=c32, v=dbl, n=n_out: (
            lambda L, h: L.spfm_interaction_topk(h, o, k, ptr(r), ptr(c), ptr(v), ptr(n))),
        "list": lambda o=0, tol=0.0, cap=64, r=r32, c=c32, v=dbl, n=n_out: (
            lambda L, h: L.spfm_interaction_list(h, o, tol, cap, ptr(r), ptr(c), ptr(v), ptr(n))),
        "values": lambda o=0, n=2, r=i32(0, 1), c=i32(1, 2), v=dbl: (
            lambda L, h: L.spfm_interaction_values(h, o, n, ptr(r), ptr(c), ptr(v))),
        "block": lambda o=0, nj=2, j=i32(0, 1), nj2=2, j2=i32(1, 2), out=dbl: (
            lambda L, h: L.spfm_interaction_block(h, o, nj, ptr(j), nj2, ptr(j2), ptr(out))),
    }
    for name, mk in ent.items():
        add("interaction_%s:null_handle" % name, None, mk())
        add("interaction_%s:no_params" % name, "data", mk())
        add("interaction_%s:order_low" % name, "fit", mk(o=-1))
        add("interaction_%s:order_high" % name, "fit", mk(o=2))
    add("interaction_stats:counts_null", "fit", ent["stats"](c=None))
    add("interaction_stats:sums_null", "fit", ent["stats"](s=None))
    add("interaction_stats:tol_negative", "fit", ent["stats"](tol=-1.0))
    add("interaction_stats:tol_nan", "fit", ent["stats"](tol=nan))
    add("interaction_topk:n_out_null", "fit", ent["topk"](n=None))
    add("interaction_topk:k_negative", "fit", ent["topk"](k=-1))
    add("interaction_topk:k_above_2^28", "fit", ent["topk"](k=(1 << 28) + 1))
    add("interaction_topk:rows_null", "fit", ent["topk"](r=None))
    add("interaction_topk:cols_null", "fit", ent["topk"](c=None))
    add("interaction_topk:vals_null", "fit", ent["topk"](v=None))
    add("interaction_list:n_out_null", "fit", ent["list"](n=None))
    add("interaction_list:tol_negative", "fit", ent["list"](tol=-1.0))
    add("interaction_list:tol_nan", "fit", ent["list"](tol=nan))
    add("interaction_list:capacity_negative", "fit", ent["list"](cap=-1))
    add("interaction_list:rows_null", "fit", ent["list"](r=None))
    add("interaction_list:capacity_short", "fit", ent["list"](cap=1))
    add("interaction_values:l_negative", "fit", ent["values"](n=-1))
    add("interaction_values:rows_null", "fit", ent["values"](r=None))
    add("interaction_values:vals_null", "fit", ent["values"](v=None))
    add("interaction_values:row_high", "fit", ent["values"](r=i32(0, D)))
    add("interaction_values:col_negative", "fit", ent["values"](c=i32(-1, 2)))
    add("interaction_block:nj_negative", "fit", ent["block"](nj=-1))
    add("interaction_block:nj2_negative", "fit", ent["block"](nj2=-1))
    add("interaction_block:j_null", "fit", ent["block"](j=None))
    add("interaction_block:j2_null", "fit", ent["block"](j2=None))
    add("interaction_block:j_high", "fit", ent["block"](j=i32(0, D)))
    add("interaction_block:j2_negative", "fit", ent["block"](j2=i32(-1, 2)))
    wide = np.zeros(11586, np.int32)  # 11586^2 doubles: just above the 2^30-byte budget
    add("interaction_block:over_budget", "fit",
        ent["block"](nj=wide.size, j=wide, nj2=wide.size, j2=wide))
    add("interaction_block:out_null", "fit", ent["block"](out=None))

    # ---- spfm_gram_csr_dense / spfm_gram_csr_csr
    B = np.ascontiguousarray(P[0])  # (K x D)
    gout = np.zeros(N * N)
    pptr, pidx, pdat = i64(0, 2, 3), i32(0, 3, 1), f64(1.0, -2.0, 0.5)

    def gd(kind=0, degree=2, n1=N, d=D, indptr=INDPTR, indices=INDICES, data=DATA, n2=K, b=B,
           lams=None, tr=0, budget=0, out=gout):
        return lambda L, h: L.spfm_gram_csr_dense(h, kind, degree, n1, d, ptr(indptr), ptr(indices),
                                                  ptr(data), n2, ptr(b), ptr(lams), tr, budget,
                                                  ptr(out))

    def gc(kind=0, degree=2, n1=N, d=D, indptr=INDPTR, indices=INDICES, data=DATA, n2=2,
           ip2=pptr, ix2=pidx, dat2=pdat, lams=None, budget=0, out=gout):
        return lambda L, h: L.spfm_gram_csr_csr(h, kind, degree, n1, d, ptr(indptr), ptr(indices),
                                                ptr(data), n2, ptr(ip2), ptr(ix2), ptr(dat2),
                                                ptr(lams), budget, ptr(out))
    for name, mk in (("gram_csr_dense", gd), ("gram_csr_csr", gc)):
        add(name + ":null_handle", None, mk())
        add(name + ":kind_unknown", "fresh", mk(kind=3))
        add(name + ":anova_degree_65", "fresh", mk(degree=65))
        add(name + ":poly_degree_negative", "fresh", mk(kind=1, degree=-1))
        add(name + ":out_null", "fresh", mk(out=None))
        add(name + ":budget_negative", "fresh", mk(budget=-1))
        add(name + ":n2_negative", "fresh", mk(n2=-1))
        add(name + ":n2_above_int32", "fresh", mk(n2=big))
        add(name + ":x_n1_negative", "fresh", mk(n1=-1))
        add(name + ":x_d_negative", "fresh", mk(d=-1))
        add(name + ":x_indptr_null", "fresh", mk(indptr=None))
        add(name + ":x_indptr0", "fresh", mk(indptr=bad_ptr0))
        add(name + ":x_indptr_decreases", "fresh", mk(indptr=not_mono))
        add(name + ":x_col_high", "fresh", mk(indices=col_hi))
        add(name + ":x_col_negative", "fresh", mk(indices=col_lo))
        add(name + ":x_unsorted", "fresh", mk(indices=unsorted))
        add(name + ":x_duplicate", "fresh", mk(indices=dup))
        add(name + ":x_data_null", "fresh", mk(data=None))
    add("gram_csr_dense:b_null", "fresh", gd(b=None))
    add("gram_csr_dense:transpose_with_lams", "fresh", gd(lams=LAMS, tr=1))
    add("gram_csr_csr:p_indptr_null", "fresh", gc(ip2=None))
    add("gram_csr_csr:p_indptr0", "fresh", gc(ip2=i64(1, 2, 3)))
    add("gram_csr_csr:p_indptr_decreases", "fresh", gc(ip2=i64(0, 2, 1)))
    add("gram_csr_csr:p_col_high", "fresh", gc(ix2=i32(0, D, 1)))
    add("gram_csr_csr:p_unsorted", "fresh", gc(ix2=i32(3, 0, 1)))
    add("gram_csr_csr:p_data_null", "fresh", gc(dat2=None))

    # ---- spfm_predict_csr
    def pr(n=N, indptr=INDPTR, indices=INDICES, degree=2, lower=0, out=dbl):
        return lambda L, h: L.spfm_predict_csr(h, n, ptr(indptr), ptr(indices), ptr(DATA), degree, 1,
                                               lower, ptr(out))
    add("predict:null_handle", None, pr())
    add("predict:no_params", "data", pr())
    add("predict:n_negative", "params", pr(n=-1))
    add("predict:indptr_null", "params", pr(indptr=None))
    add("predict:out_null", "params", pr(out=None))
    add("predict:col_high", "params", pr(indices=col_hi))
    add("predict:col_negative", "params", pr(indices=col_lo))
    add("predict:degree_1", "params", pr(degree=1))
    add("predict:degree_7", "params", pr(degree=7))
    add("predict:lower_needs_two_orders", "one_order", pr(lower=1))
    return cases


CASES = _cases()
DTYPES = ("f32", "f64")


def run_case(lib, dtype, state, call):
    """(rc, message) of one refused call on a fresh handle in `state`"""
    if state is None:
        rc = call(lib, None)
        return [int(rc), lib.spfm_last_error(None).decode()]
    if state == "one_order":
        hd = Handle(lib, dtype, "fresh")
        hd.ok(lib.spfm_set_params(hd.h, 1, K, D, ptr(np.ascontiguousarray(P[:1])), ptr(W), ptr(LAMS)))
    else:
        hd = Handle(lib, dtype, state)
    try:
        rc = call(lib, hd.h)
        return [int(rc), lib.spfm_last_error(hd.h).decode()]
    finally:
        hd.close()


def record():
    lib = _capi.load()
    return {dt: {name: run_case(lib, dt, state, call) for name, state, call in CASES}
            for dt in DTYPES}


# ====================================================================== the psgd unit
# A table of its own (python tools/record_errors.py --psgd profiles/errors_psgd_parent_<sha>.json):
# every refusal that a small pair problem can reach in spfm_psgd_epoch, spfm_psgd_epoch_sharded (no
# communicator: its argument checks only), spfm_psgd_pairs_epoch, spfm_psgd_pairs_eval,
# spfm_psgd_pairs_set_sampler, spfm_psgd_pairs_sample and spfm_psgd_pairs_epoch_sampled.  6 context
# rows (columns 0..4) over 5 candidate rows (columns 5..8), k = 2.  (Not reachable at this size:
# more than 2^31 - 1 positives, and everything behind a communicator.)
PS_NCTX, PS_NCAND, PS_D, PS_K = 6, 5, 9, 2
PS_N = PS_NCTX + PS_NCAND


def _psgd_problem():
    rng = np.random.RandomState(11)
    dense = np.zeros((PS_N, PS_D))
    for i in range(PS_N):
        cols = np.arange(0, 5) if i < PS_NCTX else np.arange(5, PS_D)
        pick = rng.choice(cols, 2, replace=False)
        dense[i, pick] = rng.randn(2)
    shared = dense.copy()
    shared[PS_NCTX + 1, np.flatnonzero(dense[0])[0]] = 0.5  # a column of context 0 in candidate 1

    def csr(a):
        indptr = np.zeros(PS_N + 1, np.int64)
        indices, data = [], []
        for i in range(PS_N):
            nzc = np.flatnonzero(a[i])
            indices += list(nzc)
            data += list(a[i, nzc])
            indptr[i + 1] = len(indices)
        return indptr, np.asarray(indices, np.int32), np.asarray(data, np.float64)

    return (csr(dense), csr(shared), np.zeros(PS_N), 0.1 * rng.randn(1, PS_K, PS_D),
            0.1 * rng.randn(PS_D), np.ones(PS_K))


PS_X, PS_XSHARED, PS_Y, PS_P, PS_W, PS_LAMS = _psgd_problem()
# positives: every context but 4 has some; forbidden = positives + one more in rows 0 and 2
PS_POS_PTR, PS_POS_IDX = i64(0, 2, 3, 4, 6, 6, 7), i32(0, 3, 1, 2, 0, 4, 3)
PS_FORB_PTR, PS_FORB_IDX = i64(0, 3, 4, 6, 8, 8, 9), i32(0, 2, 3, 1, 2, 4, 0, 4, 3)
PS_NPOS = int(PS_POS_PTR[-1])
PS_TRIPLES = i32(0, 6, 7, 1, 8, 6, 5, 10, 9)  # three valid triples (context, plus, minus)
PS_STEP = (0.01, 0.5, 0.003, 0.05)  # alpha, beta, gamma, eta0


class PsgdHandle:
    """A fresh handle brought to a named state by calls that all succeed."""

    STEPS = {
        "fresh": "", "data": "d", "unconfigured": "dp", "pcd": "dpc", "psgd": "dpg",
        "shared": "Dpg", "sampler": "dpgs", "sampled": "dpgsS", "sampled_eval": "dpgsSe",
        "sampled_epoch": "dpgsSu", "pcd_sampler": "dpcs",
    }

    def __init__(self, lib, dtype, state):
        self.lib = lib
        self.h = C.c_void_p()
        assert lib.spfm_create(C.byref(self.h), 0, _capi.DTYPES[dtype]) == 0
        for s in self.STEPS[state]:
            getattr(self, "_" + s)()

    def ok(self, rc):
        assert rc == 0, (rc, self.lib.spfm_last_error(self.h))

    def _data(self, X):
        self.ok(self.lib.spfm_set_data_csr(self.h, PS_N, PS_D, ptr(X[0]), ptr(X[1]), ptr(X[2]),
                                           ptr(PS_Y)))

    def _d(self):
        self._data(PS_X)

    def _D(self):
        self._data(PS_XSHARED)

    def _p(self):
        self.ok(self.lib.spfm_set_params(self.h, 1, PS_K, PS_D, ptr(PS_P), ptr(PS_W), ptr(PS_LAMS)))

    def _configure(self, solver):
        self.ok(self.lib.spfm_configure(self.h, _capi.SOLVERS[solver], _capi.LOSSES["logistic"],
                                        _capi.REGULARIZERS["l1"], 2))

    def _c(self):
        self._configure("pcd")

    def _g(self):
        self._configure("psgd")

    def _s(self):
        self.ok(self.lib.spfm_psgd_pairs_set_sampler(self.h, PS_NCTX, PS_NCAND, ptr(PS_POS_PTR),
                                                     ptr(PS_POS_IDX), ptr(PS_FORB_PTR),
                                                     ptr(PS_FORB_IDX)))

    def _S(self):
        self.ok(self.lib.spfm_psgd_pairs_sample(self.h, 2, 1, 1, 16, 1, 0, NULL, NULL, NULL))

    def _e(self):
        self.ok(self.lib.spfm_psgd_pairs_eval(self.h, 2, 1, ptr(PS_TRIPLES), 3, NULL, NULL))

    def _u(self):
        it = i64(1)
        self.ok(self.lib.spfm_psgd_pairs_epoch(self.h, 2, *PS_STEP, 1, 0.8, 2, ptr(PS_TRIPLES), 3,
                                               1, ptr(it), NULL))

    def close(self):
        self.lib.spfm_destroy(self.h)


def _psgd_cases():
    """(name, state, call(lib, h) -> rc); `h` is None for the NULL-handle cases"""
    cases = []
    big = 1 << 31
    perm = np.arange(PS_N, dtype=np.int32)[::-1].copy()
    preamble = ("fresh", "data", "unconfigured", "pcd")

    def add(name, state, call):
        cases.append((name, state, call))

    def tri(*rows):
        return i32(*rows)

    def with_(a, pos, v):
        b = a.copy()
        b[pos] = v
        return b

    not_perm = (("repeat", lambda a: with_(a, 1, a[0])), ("negative", lambda a: with_(a, 2, -1)),
                ("entry_m", lambda a: with_(a, 0, a.size)))

    # ---- spfm_psgd_epoch / spfm_psgd_epoch_sharded (no communicator)
    def ep(degree=2, lr=1, batch=4, order=perm, n=PS_N, it=1, with_it=True, row_lo=None):
        def call(L, h):
            itv = i64(it)
            head = (h, degree) + PS_STEP + (lr, 0.8, batch, ptr(order), n)
            tail = (1, ptr(itv) if with_it else NULL, NULL)
            if row_lo is None:
                return L.spfm_psgd_epoch(*(head + tail))
            return L.spfm_psgd_epoch_sharded(*(head + (row_lo,) + tail))
        return call
    for ent, kw in (("psgd_epoch", {}), ("psgd_epoch_sharded", dict(row_lo=0))):
        add(ent + ":null_handle", None, ep(**kw))
        for st in preamble:
            add(ent + ":state_" + st, st, ep(**kw))
        add(ent + ":degree_differs", "psgd", ep(degree=3, **kw))
        add(ent + ":indices_null", "psgd", ep(order=None, **kw))
        add(ent + ":it_null", "psgd", ep(with_it=False, **kw))
        add(ent + ":n_samples_differs", "psgd", ep(n=PS_N - 1, **kw))
        add(ent + ":batch_size_0", "psgd", ep(batch=0, **kw))
        add(ent + ":learning_rate_negative", "psgd", ep(lr=-1, **kw))
        add(ent + ":learning_rate_4", "psgd", ep(lr=4, **kw))
        add(ent + ":it_0", "psgd", ep(it=0, **kw))
        for nm, mk in not_perm:
            add(ent + ":not_a_permutation_" + nm, "psgd", ep(order=mk(perm), **kw))
    add("psgd_epoch_sharded:row_lo_1", "psgd", ep(row_lo=1))
    add("psgd_epoch_sharded:row_lo_negative", "psgd", ep(row_lo=-1))

    # ---- the triples of spfm_psgd_pairs_epoch / spfm_psgd_pairs_eval
    def pe(degree=2, lr=1, batch=2, triples=PS_TRIPLES, m=3, it=1, with_it=True):
        def call(L, h):
            itv = i64(it)
            return L.spfm_psgd_pairs_epoch(h, degree, *PS_STEP, lr, 0.8, batch, ptr(triples), m, 1,
                                           ptr(itv) if with_it else NULL, NULL)
        return call

    def pv(degree=2, triples=PS_TRIPLES, m=3, **_):
        return lambda L, h: L.spfm_psgd_pairs_eval(h, degree, 1, ptr(triples), m, NULL, NULL)
    for ent, mk in (("pairs_epoch", pe), ("pairs_eval", pv)):
        add(ent + ":null_handle", None, mk())
        for st in preamble:
            add(ent + ":state_" + st, st, mk())
        add(ent + ":degree_differs", "psgd", mk(degree=3))
        add(ent + ":m_negative", "psgd", mk(m=-1))
        add(ent + ":triples_null", "psgd", mk(triples=None))
        add(ent + ":m_2^31", "psgd", mk(m=big))
        add(ent + ":anchor_negative", "psgd", mk(triples=tri(0, 6, 7, -1, 8, 6, 5, 10, 9)))
        add(ent + ":anchor_n", "psgd", mk(triples=tri(PS_N, 6, 7, 1, 8, 6, 5, 10, 9)))
        add(ent + ":plus_n", "psgd", mk(triples=tri(0, 6, 7, 1, PS_N, 6, 5, 10, 9)))
        add(ent + ":plus_negative", "psgd", mk(triples=tri(0, -3, 7, 1, 8, 6, 5, 10, 9)))
        add(ent + ":minus_n", "psgd", mk(triples=tri(0, 6, 7, 1, 8, 6, 5, 10, PS_N)))
        add(ent + ":minus_negative", "psgd", mk(triples=tri(0, 6, -1, 1, 8, 6, 5, 10, 9)))
        add(ent + ":plus_is_minus", "psgd", mk(triples=tri(0, 6, 7, 1, 8, 8, 5, 10, 9)))
        add(ent + ":shared_column", "shared", mk())
        # a context row as a candidate: its columns are stored on both sides
        add(ent + ":context_as_candidate", "psgd", mk(triples=tri(0, 6, 7, 1, 8, 0, 5, 10, 9)))
    add("pairs_epoch:it_null", "psgd", pe(with_it=False))
    add("pairs_epoch:batch_size_0", "psgd", pe(batch=0))
    add("pairs_epoch:learning_rate_negative", "psgd", pe(lr=-1))
    add("pairs_epoch:learning_rate_4", "psgd", pe(lr=4))
    add("pairs_epoch:it_0", "psgd", pe(it=0))

    # ---- spfm_psgd_pairs_set_sampler
    def ss(n_ctx=PS_NCTX, n_cand=PS_NCAND, pp=PS_POS_PTR, pi=PS_POS_IDX, fp=PS_FORB_PTR,
           fi=PS_FORB_IDX):
        return lambda L, h: L.spfm_psgd_pairs_set_sampler(h, n_ctx, n_cand, ptr(pp), ptr(pi),
                                                          ptr(fp), ptr(fi))
    add("set_sampler:null_handle", None, ss())
    add("set_sampler:no_data", "fresh", ss())
    add("set_sampler:n_ctx_0", "psgd", ss(n_ctx=0, n_cand=PS_N))
    add("set_sampler:n_cand_0", "psgd", ss(n_ctx=PS_N, n_cand=0))
    add("set_sampler:rows_differ", "psgd", ss(n_ctx=PS_NCTX - 1))
    for side, ip, ix in (("positives", PS_POS_PTR, PS_POS_IDX), ("forbidden", PS_FORB_PTR, PS_FORB_IDX)):
        def sd(indptr=ip, indices=ix, side=side):
            if side == "positives":  # (no forbidden set: the positives stand in for it)
                return ss(pp=indptr, pi=indices, fp=None, fi=None)
            return ss(fp=indptr, fi=indices)
        if side == "positives":
            add("set_sampler:positives:indptr_null", "psgd", sd(indptr=None))
        add("set_sampler:%s:indptr0" % side, "psgd", sd(indptr=with_(ip, 0, 1)))
        add("set_sampler:%s:indptr_not_monotone" % side, "psgd", sd(indptr=with_(ip, 2, ip[1] - 1)))
        add("set_sampler:%s:indices_null" % side, "psgd", sd(indices=None))
        add("set_sampler:%s:index_negative" % side, "psgd", sd(indices=with_(ix, 0, -1)))
        add("set_sampler:%s:index_n_cand" % side, "psgd", sd(indices=with_(ix, 1, PS_NCAND)))
        add("set_sampler:%s:repeat" % side, "psgd", sd(indices=with_(ix, 1, ix[0])))
        add("set_sampler:%s:descending" % side, "psgd",
            sd(indices=with_(with_(ix, 0, ix[1]), 1, ix[0])))
    add("set_sampler:no_positive", "psgd",
        ss(pp=np.zeros(PS_NCTX + 1, np.int64), pi=None, fp=None, fi=None))
    add("set_sampler:forbidden_lacks_a_positive", "psgd",
        ss(fp=i64(0, 3, 4, 6, 8, 8, 9), fi=i32(0, 2, 3, 1, 3, 4, 0, 4, 3)))
    add("set_sampler:forbidden_lacks_the_last_positive", "psgd",
        ss(fp=i64(0, 3, 4, 6, 7, 7, 8), fi=i32(0, 2, 3, 1, 2, 4, 0, 3)))
    # row 4 has no positive: all five candidates forbidden there is accepted; row 3 with four of
    # five is accepted too (PS_FORB has two); all five in row 3 is refused
    add("set_sampler:row_forbids_every_candidate", "psgd",
        ss(fp=i64(0, 3, 4, 6, 11, 11, 12), fi=i32(0, 2, 3, 1, 2, 4, 0, 1, 2, 3, 4, 3)))
    add("set_sampler:shared_column", "shared", ss())

    # ---- spfm_psgd_pairs_sample
    order = np.arange(PS_NPOS, dtype=np.int32)[::-1].copy()

    def sa(degree=2, n_neg=1, n_cand=2, max_draws=16, seed=1, epoch=0, order=None):
        return lambda L, h: L.spfm_psgd_pairs_sample(h, degree, n_neg, n_cand, max_draws, seed,
                                                     epoch, ptr(order), NULL, NULL)
    add("pairs_sample:null_handle", None, sa())
    for st in preamble:
        add("pairs_sample:state_" + st, st, sa())
    add("pairs_sample:state_pcd_with_sampler", "pcd_sampler", sa())
    add("pairs_sample:degree_differs", "sampler", sa(degree=3))
    add("pairs_sample:before_set_sampler", "psgd", sa())
    add("pairs_sample:n_negatives_0", "sampler", sa(n_neg=0))
    add("pairs_sample:n_candidates_0", "sampler", sa(n_cand=0))
    add("pairs_sample:max_draws_0", "sampler", sa(max_draws=0))
    add("pairs_sample:n_candidates_2^31", "sampler", sa(n_cand=big))
    add("pairs_sample:max_draws_2^31", "sampler", sa(max_draws=big))
    add("pairs_sample:n_negatives_2^31", "sampler", sa(n_neg=big))
    add("pairs_sample:list_above_2^31", "sampler", sa(n_neg=1 << 30))
    add("pairs_sample:seed_negative", "sampler", sa(seed=-1))
    add("pairs_sample:epoch_negative", "sampler", sa(epoch=-1))
    for nm, mk in not_perm:
        add("pairs_sample:order_not_a_permutation_" + nm, "sampler", sa(order=mk(order)))

    # ---- spfm_psgd_pairs_epoch_sampled
    def es(degree=2, lr=1, batch=2, it=1, with_it=True):
        def call(L, h):
            itv = i64(it)
            return L.spfm_psgd_pairs_epoch_sampled(h, degree, *PS_STEP, lr, 0.8, batch, 1,
                                                   ptr(itv) if with_it else NULL, NULL)
        return call
    add("epoch_sampled:null_handle", None, es())
    for st in preamble:
        add("epoch_sampled:state_" + st, st, es())
    add("epoch_sampled:degree_differs", "sampled", es(degree=3))
    add("epoch_sampled:before_set_sampler", "psgd", es())
    add("epoch_sampled:before_sample", "sampler", es())
    add("epoch_sampled:after_eval_upload", "sampled_eval", es())
    add("epoch_sampled:after_epoch_upload", "sampled_epoch", es())
    add("epoch_sampled:it_null", "sampled", es(with_it=False))
    add("epoch_sampled:batch_size_0", "sampled", es(batch=0))
    add("epoch_sampled:learning_rate_negative", "sampled", es(lr=-1))
    add("epoch_sampled:learning_rate_4", "sampled", es(lr=4))
    add("epoch_sampled:it_0", "sampled", es(it=0))
    return cases


PSGD_CASES = _psgd_cases()


def run_psgd_case(lib, dtype, state, call):
    """(rc, message) of one refused call on a fresh handle in `state`"""
    if state is None:
        rc = call(lib, None)
        return [int(rc), lib.spfm_last_error(None).decode()]
    hd = PsgdHandle(lib, dtype, state)
    try:
        rc = call(lib, hd.h)
        return [int(rc), lib.spfm_last_error(hd.h).decode()]
    finally:
        hd.close()


def record_psgd():
    lib = _capi.load()
    return {dt: {name: run_psgd_case(lib, dt, state, call) for name, state, call in PSGD_CASES}
            for dt in DTYPES}


def main(argv):
    if len(argv) > 1 and argv[1] == "--psgd":
        res = {"build_tag": _capi.build_tag(), "n_ctx": PS_NCTX, "n_cand": PS_NCAND, "d": PS_D,
               "k": PS_K, "cases": record_psgd()}
        refused = sum(rc != 0 for per in res["cases"].values() for rc, _ in per.values())
        with open(argv[2], "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
        print("recorded %d psgd cases per storage type, %d refusals in all"
              % (len(PSGD_CASES), refused), file=sys.stderr)
        return
    res = {"build_tag": _capi.build_tag(), "n": N, "d": D, "k": K, "cases": record()}
    refused = sum(rc != 0 for per in res["cases"].values() for rc, _ in per.values())
    text = json.dumps(res, indent=1, sort_keys=True)
    if len(argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(argv[1])), exist_ok=True)
        with open(argv[1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    print("recorded %d cases per storage type, %d refusals in all" % (len(CASES), refused),
          file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv)
