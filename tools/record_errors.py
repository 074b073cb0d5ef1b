"""Drive one handle per storage type through a fixed table of refused calls and write
``(return code, spfm_last_error)`` per case to JSON.

    python tools/record_errors.py profiles/errors_parent_<sha>.json

The table covers every argument check (FAIL or bare SPFM_ERR_INVALID) that inputs of n = 8, d = 5,
k = 2 can reach in spfm_set_data_csr, spfm_set_data_csc, spfm_set_eval_csr, spfm_eval_loss,
spfm_objective_terms, the five spfm_interaction_* entries, the two spfm_gram_* entries and
spfm_predict_csr.  (Not reachable at this size: the tie bound of interaction_topk, which needs
more than 2^20 candidates, and the internal consistency checks that answer SPFM_ERR_RUNTIME.)
tests/test_hip_errors.py replays the table against the recording of the parent commit.
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


def main(argv):
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
