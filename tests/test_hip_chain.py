"""The production chains of the pcd passes (pcd_chain_lanes, pcd_chain_waves; csrc/spfm_pcd.hip.h),
run by HipEngine.debug_chain on the cases of tests/test_chain_host.py and measured, column by
column, against that file's exact rational reference -- never against another device form.

Per case: the set of zeroed columns and the signs of the others equal the reference's; values and
the final cache lie inside the bound below; the omegati clip counter ticks exactly when the
reference clips; the same call twice returns the same bits.  For ncols <= 64 at degree 2 the
one-wave and the wide form return the same bits.

The bound (u = 2^-53; nothing in it was fitted to the device).  The exact reference carries a
first-order running error bound e (units of u) through its own recurrence:
  * step-size block: inv = h mu + beta (2 roundings), the numerator g lam + beta p (<= 2 u of its
    absolute terms), recip_nr (<= 1.5 ulp = 3 u), three more products and sums: the error of p_in
    is at most 10 u (T + |p_in|) with T = eta (|g lam| + |beta p|) / inv; of the strength 7 u
    relative; squaredl12's pre-scaling by recip_nr(1 + 2 s) adds 6 u to |p_in| / (1 + 2 s) and
    makes 13 u relative for 2 s / (1 + 2 s);
  * every later operation adds one rounding of its result and passes its operands' errors on with
    the operation's own derivatives (max(., 0) is 1-Lipschitz): for m = p - s d that is
    e_p + e_s d + s e_d + |s d| + |m|, and likewise along the cache recurrences.
That covers a sequential evaluation.  The speculative forms evaluate the same exact function of
the same inputs in another association, which adds:
  * degree-2 scans (squaredl12, omegati): the cache in front of a column is A c0 + B with (A, B)
    a prefix composition over L levels, each level be = al * ob + be (2 roundings), al = al * oa
    (1).  With |al| <= 1 for the final branches (asserted in the host file) the error of B is at
    most 2 L u W and of A at most L u, W = |c0| + sum_k (|p_in,k'| + |p_old,k|) bounding every
    partial B; with the two roundings of A c0 + B: 3 L u W.  L = 6 for the one-wave form, 6 + 8
    for the wide form (a wave's input and the final cache pass through up to 8 wave maps);
  * degree 3: the two caches in front of a column are prefix sums over the same 6 levels plus the
    offset, 7 u W1 and 7 u W2 with W1 = |c1| + sum |r - a|, W2 = |c2| + sum |dc2 (r - a)|; they
    reach m through s (dc3 = c2 - dc2 a) and every non-zero column feeds its error into the sums
    once more: 7 (W2 + a_max W1) max(s_max, 1) (1 + number of non-zero columns).
The tolerance of a coordinate is u (2 (e_i + extra) + scale) -- the factor 2 for second-order terms
and the reassociated roundings, `scale` (the largest magnitude of the case) for the final rounding
-- and the same with the largest cache bound for the cache.  The plain sequential float64
restatement stays inside the same bound without the extra terms (host file).  Cases built from
small dyadic numbers (exact ties) are compared for equality: recip_nr(1) and recip_nr(2) are exact
after their Newton steps.

Not covered: feeding a production step's own column sums to the probe (the multi-kernel engine
has no getter for them, and the hot kernels get no read-outs for a test).

GPU tests need a real MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

import test_chain_host as H

U = H.U
WORST = {}


@pytest.fixture(scope="module")
def engine():
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    yield eng
    eng.close()


def _run(engine, c, form=None):
    return engine.debug_chain(c["form"] if form is None else form, c["reg"], c["degree"],
                              c["p_old"], c["g"], c["h"], c["lam"], c["mu"], c["beta"],
                              c["gamma"], c["eta"], c["cache_in"][:c["degree"] + 1])


def _scheme(c):
    if c["reg"] == "l1":
        return "l1"
    if c["degree"] == 2:
        return ("wide-" if c["form"] == 1 else "scan-") + c["reg"]
    return {3: "degree3", 0: "all-subsets"}.get(c["degree"], "serial")


def extra_terms(c, ex):
    """association terms of the speculative forms, units of u (module docstring)"""
    if c["reg"] == "l1":
        return 0.0
    ab, app, tt, _ = H._lane_constants(c, 0, len(c["p_old"]))
    if c["degree"] == 2:
        c0 = abs(float(c["cache_in"][0 if c["reg"] == "squaredl12" else 1]))
        L = 14 if c["form"] == 1 else 6
        return 3.0 * L * (c0 + float((app + ab).sum()))
    if c["degree"] == 3:
        r = np.array([abs(float(v)) for v in ex["p"]])
        d1 = r - ab
        c1 = float(c["cache_in"][1]) + np.concatenate(([0.0], np.cumsum(d1)[:-1]))
        dc2 = np.maximum(c1 - ab, 0.0)
        W1 = abs(float(c["cache_in"][1])) + float(np.abs(d1).sum())
        W2 = abs(float(c["cache_in"][2])) + float(np.abs(dc2 * d1).sum())
        return 7.0 * (W2 + float(ab.max()) * W1) * max(float(tt.max()), 1.0) * (1 + int((r > 0).sum()))
    return 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("cid", H.case_ids())
def test_chain_case(engine, cid):
    c = H.case_by_id(cid)
    ex = H.exact_of(c.get("twin_of", cid))
    engine.debug_branch_counts(reset=True)
    p, cache = _run(engine, c)
    clips = engine.debug_branch_counts(reset=True)["omegati_clip"]
    p2, cache2 = _run(engine, c)
    # 5. determinism
    assert p.tobytes() == p2.tobytes() and cache.tobytes() == cache2.tobytes()
    want = np.array([float(v) for v in ex["p"]])
    want_c = np.array([float(v) for v in ex["cache"]])[:c["degree"] + 1]
    # 1. branches: zero set and signs
    assert ((p == 0) == (want == 0)).all(), np.nonzero((p == 0) != (want == 0))[0]
    nzc = want != 0
    assert (np.sign(p[nzc]) == np.sign(want[nzc])).all()
    # 4. path evidence
    assert clips == (1 if ex["clipped"] else 0), (clips, ex["clipped"])
    # 2. values
    if c["exact"]:
        assert (np.abs(p) == np.abs(want)).all() and (cache == want_c).all()
        return
    extra = extra_terms(c, ex)
    tol_p = U * (2.0 * (ex["err_p"] + extra) + ex["scale"])
    tol_c = U * (2.0 * (ex["err_c"] + extra) + ex["scale"])
    fl, fc = H.float_chain(c)
    rp = float((np.abs(p - want) / tol_p).max())
    rc = float((np.abs(cache - want_c) / tol_c).max())
    rb = float((np.abs(fl - want) / tol_p).max())
    print("%s: device error / bound %.3e (p) %.3e (cache); baseline / bound %.3e" % (cid, rp, rc, rb))
    w = WORST.setdefault(_scheme(c), [0.0, 0.0])
    w[0], w[1] = max(w[0], rp, rc), max(w[1], rb)
    assert rp <= 1.0 and rc <= 1.0, (rp, rc)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in H.cases() if "twin_of" in c])
def test_forms_agree_bitwise(engine, cid):
    """ncols <= 64, degree 2: the wide chain returns the bits of the one-wave chain (the claim of
    the comment above pcd_chain_waves)"""
    c = H.case_by_id(cid)
    p0, c0 = _run(engine, c, form=0)
    p1, c1 = _run(engine, c, form=1)
    assert p0.tobytes() == p1.tobytes() and c0.tobytes() == c1.tobytes()


@pytest.mark.gpu
def test_invalid_arguments(engine):
    z = np.zeros(4)
    ok = dict(form=0, regularizer="omegati", degree=3, p_old=z, g=z, hsum=z + 1, lam=1, mu=1, beta=0,
              gamma=0, eta=1, cache_in=np.zeros(4))
    engine.debug_chain(**ok)
    for bad in (dict(form=2), dict(regularizer="l21"), dict(regularizer="omegacs"),
                dict(degree=7, cache_in=np.zeros(8)), dict(degree=1, cache_in=np.zeros(2)),
                dict(regularizer="squaredl12"), dict(form=1),
                dict(p_old=np.zeros(0), g=np.zeros(0), hsum=np.zeros(0)),
                dict(p_old=np.zeros(65), g=np.zeros(65), hsum=np.ones(65)),
                dict(form=1, degree=2, cache_in=np.zeros(3), p_old=np.zeros(513), g=np.zeros(513),
                     hsum=np.ones(513))):
        with pytest.raises(ValueError):
            engine.debug_chain(**dict(ok, **bad))


@pytest.mark.gpu
def test_zz_worst_ratios():
    """prints the worst observed ratios per scheme (recorded in DESIGN.md)"""
    for k in sorted(WORST):
        print("worst %-18s device/bound %.3e  baseline/bound %.3e" % (k, WORST[k][0], WORST[k][1]))
    assert all(v[0] <= 1.0 for v in WORST.values())
