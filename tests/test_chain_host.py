"""The chain of a dependent pcd step -- step size, prox, regularizer-cache recurrence (reference
pcd.py:61-68 with prox_cd / update_cache_pcd of l1, squaredl12 and omegati) -- column by column:
the exact reference, a host emulation of the device's speculative schemes, and the cases that
tests/test_hip_chain.py feeds to the production device chains (HipEngine.debug_chain).  No GPU.

1. ``exact_chain``: the recurrences in ``fractions.Fraction`` (only + - * /, abs and max occur),
   columns one after the other in the reference's order, clips included.  It returns the new
   coordinates, the final cache, every decision (``m > 0``, every clip argument ``v >= 0``) and a
   first-order running error bound in units of 2^-53 (derived in tests/test_hip_chain.py).  It is
   checked here against the float64 host face sparsepoly_amd/regularizer.py.
2. ``emulate``: NumPy restatements of the three speculative schemes of csrc/spfm_pcd.hip.h -- the
   affine prefix scan over DPP moves with its re-check rounds, the degree-3 fixed point with its
   8-round cap and serial fallback, the wave-level repeat of the wide chain.  They only COUNT
   rounds and predict the path a case takes; values are never compared with them.
3. ``cases()``: the generator.  Every generic case keeps a relative margin CLEAR = 1e-9 of the
   case's scale at every decision of the exact reference (the convention of
   tests/test_hip_interactions.py), so which columns end at zero is a property of the input and
   not of rounding.  The tests below assert the column counts, margins, round counts and predicted
   paths the cases exist for, so that the GPU file cannot drift into easy inputs.
"""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest

U = 2.0 ** -53
CLEAR = 1e-9
WAVE = 64

LANES_NCOLS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
SERIAL_LAST = (0, 2, 3, 4, 7, 8, 62, 63)
WAVES_NCOLS = (63, 64, 65, 127, 128, 129, 448, 449, 511, 512)


# ------------------------------------------------------------------ exact reference
def exact_chain(case):
    """Sequential chain in exact rational arithmetic.  Returns dict: p (Fractions), cache
    (Fractions, degree + 1 entries; entries the chain does not own copied through), dec (per column:
    dict m=Fraction, v=[clip arguments]), clipped (bool), err_p / err_c (running first-order error
    bounds of the coordinates / of any cache value, units of 2^-53, floats), scale."""
    reg, M = case["reg"], case["degree"]
    F = lambda x: Fr(float(x))
    lam, mu, beta, gamma, eta = (F(case[k]) for k in ("lam", "mu", "beta", "gamma", "eta"))
    c = [F(v) for v in case["cache_in"]]
    ec = [0.0] * len(c)            # running error bounds of the cache entries
    out, dec, err_p = [], [], []
    scale = max([abs(float(v)) for v in c] + [0.0])
    clipped = False
    for p_f, g_f, h_f in zip(case["p_old"], case["g"], case["h"]):
        p, g, h = F(p_f), F(g_f), F(h_f)
        inv = h * mu + beta
        pin = p - eta * ((g * lam + beta * p) / inv)
        st = eta * gamma / inv
        a = abs(p)
        T = float(eta * (abs(g * lam) + abs(beta * p)) / inv)
        fpin, fst, fa = abs(float(pin)), float(st), float(a)
        e_pin = 10.0 * (T + fpin)      # recip_nr (3) + inv (2) + numerator (2) + 3 products/sums
        e_st = 7.0 * fst
        scale = max(scale, fa, fpin, T)
        d = {"v": []}
        if reg == "l1":
            m = abs(pin) - st
            r = max(m, Fr(0))
            sg = 1 if pin > 0 else (-1 if pin < 0 else 0)
            e = e_pin + e_st + abs(float(m))
        elif reg == "squaredl12":
            den = 1 + 2 * st
            app, tt = abs(pin) / den, 2 * st / den
            fapp, ftt = float(app), float(tt)
            e_app, e_tt = e_pin / float(den) + 6.0 * fapp, 13.0 * ftt
            v = c[0] - a
            e_v = ec[0] + abs(float(v))
            m = app - tt * v
            e = e_app + e_tt * abs(float(v)) + ftt * e_v + abs(float(tt * v)) + abs(float(m))
            r = max(m, Fr(0))
            sg = 1 if pin > 0 else -1
            c[0] = v + r
            ec[0] = e_v + (e if r > 0 else 0.0) + abs(float(c[0]))
        elif M == 0:  # omegati, all-subsets
            c[0] = c[0] / (1 + a)
            ec[0] = ec[0] / (1.0 + fa) + 2.0 * float(c[0])
            m = abs(pin) - st * c[0]
            e = e_pin + e_st * float(c[0]) + fst * ec[0] + float(st * c[0]) + abs(float(m))
            r = max(m, Fr(0))
            sg = 1 if pin > 0 else -1
            c[0] = c[0] * (1 + r)
            ec[0] = ec[0] * float(1 + r) + float(c[0]) * 2.0 + (float(c[0]) * e if r > 0 else 0.0)
        else:         # omegati, degree M
            dc, edc = [None, Fr(1)], [0.0, 0.0]
            for t in range(2, M + 1):
                v = c[t - 1] - dc[t - 1] * a
                d["v"].append(v)
                if v < 0:
                    clipped = True
                edc.append(ec[t - 1] + edc[t - 1] * fa + float(dc[t - 1] * a) + abs(float(v)))
                dc.append(max(v, Fr(0)))
            m = abs(pin) - st * dc[M]
            fd = float(dc[M])
            e = e_pin + e_st * fd + fst * edc[M] + fst * fd + abs(float(m))
            r = max(m, Fr(0))
            sg = 1 if pin > 0 else -1
            er, fr = (e if r > 0 else 0.0), float(r)
            for t in range(1, M):
                c[t] = dc[t + 1] + dc[t] * r
                ec[t] = (edc[t + 1] + edc[t] * fr + float(dc[t]) * er + float(dc[t] * r)
                         + float(c[t]))
        d["m"] = m
        dec.append(d)
        out.append(sg * r)
        err_p.append(e)
        scale = max([scale] + [abs(float(v)) for v in c])
    return dict(p=out, cache=c, dec=dec, clipped=clipped, err_p=np.array(err_p),
                err_c=max(ec + [0.0]), scale=scale)


def margin(case, ex):
    """smallest |decision value| of the exact chain, relative to the case's scale"""
    vals = []
    for d in ex["dec"]:
        vals.append(abs(d["m"]))
        vals.extend(abs(v) for v in d["v"])
    return float(min(vals)) / ex["scale"]


def float_chain(case):
    """The same chain in plain sequential float64 (the baseline whose error the bound must cover):
    pcd.py:61-68 followed by the host face's prox_cd / update_cache_pcd formulas."""
    reg, M = case["reg"], case["degree"]
    lam, mu, beta, gamma, eta = (float(case[k]) for k in ("lam", "mu", "beta", "gamma", "eta"))
    c = [float(v) for v in case["cache_in"]]
    out = []
    for p, g, h in zip(case["p_old"], case["g"], case["h"]):
        p, g, h = float(p), float(g), float(h)
        inv = h * mu + beta
        upd = (g * lam + beta * p) / inv
        pin = p - eta * upd
        st = eta * gamma / inv
        a = abs(p)
        if reg == "l1":
            r = float(np.sign(pin)) * max(abs(pin) - st, 0.0)
        elif reg == "squaredl12":
            others = c[0] - a
            pp = pin / (1.0 + 2.0 * st)
            r = (1.0 if pp > 0 else -1.0) * max(abs(pp) - 2.0 * st * others / (1.0 + 2.0 * st), 0.0)
            c[0] = others + abs(r)
        elif M == 0:
            c[0] /= 1.0 + a
            r = (1.0 if pin > 0 else -1.0) * max(abs(pin) - st * c[0], 0.0)
            c[0] *= 1.0 + abs(r)
        else:
            dc = [0.0, 1.0]
            for t in range(2, M + 1):
                dc.append(max(c[t - 1] - dc[t - 1] * a, 0.0))
            r = (1.0 if pin > 0 else -1.0) * max(abs(pin) - st * dc[M], 0.0)
            for t in range(1, M):
                c[t] = dc[t + 1] + dc[t] * abs(r)
        out.append(r)
    return np.array(out), np.array(c)


# ------------------------------------------------------------------ host emulation
def _dpp_sources():
    """source lane (or -1: keep `old`) of every lane for the six moves of affine_scan_inclusive:
    row_shr:1/2/4/8 inside rows of 16, row_bcast:15 into rows 1 and 3, row_bcast:31 into 2 and 3"""
    lanes = np.arange(WAVE)
    moves = []
    for n in (1, 2, 4, 8):
        moves.append(np.where((lanes & 15) >= n, lanes - n, -1))
    moves.append(np.where((lanes >> 4) % 2 == 1, (lanes & ~15) - 1, -1))
    moves.append(np.where(lanes >= 32, 31, -1))
    return moves


_MOVES = _dpp_sources()


def affine_scan_inclusive(al, be, moves=_MOVES):
    al, be = al.copy(), be.copy()
    for src in moves:
        oa = np.where(src >= 0, al[np.maximum(src, 0)], 1.0)
        ob = np.where(src >= 0, be[np.maximum(src, 0)], 0.0)
        be = al * ob + be
        al = al * oa
    return al, be


def affine_before(al, be, c0):
    pa = np.concatenate(([0.0], al[:-1]))
    pb = np.concatenate(([c0], be[:-1]))
    return pa * c0 + pb


def _lane_constants(case, lo=0, n=WAVE):
    """per-lane float64 operands of columns lo .. lo + n - 1, padded to n lanes"""
    sl = slice(lo, lo + n)
    p, g, h = (np.asarray(case[k], dtype=np.float64)[sl] for k in ("p_old", "g", "h"))
    k = p.size
    inv = h * case["mu"] + case["beta"]
    pin = p - case["eta"] * ((g * case["lam"] + case["beta"] * p) / inv)
    st = case["eta"] * case["gamma"] / inv
    if case["reg"] == "squaredl12":
        den = 1.0 + 2.0 * st
        app, tt = np.abs(pin / den), 2.0 * st / den
    else:
        app, tt = np.abs(pin), st
    pad = lambda v: np.concatenate((v, np.zeros(n - k)))
    act = np.arange(n) < k
    return pad(np.abs(p)), pad(app), pad(tt), act


class _Deg2Wave(object):
    """one wave of the degree-2 scan: branch state (pos, nz) and the scan of its maps"""

    def __init__(self, case, lo):
        self.sq = case["reg"] == "squaredl12"
        self.ab, self.app, self.tt, self.act = _lane_constants(case, lo)
        self.first_bad = []

    def guess(self, c0):
        self.pos = np.ones(WAVE, bool) if self.sq else (c0 - self.ab) >= 0
        self.nz = (self.app - self.tt * np.where(self.pos, c0 - self.ab, 0.0)) > 0
        self.scan()

    def scan(self):
        al = np.where(~self.act, 1.0, np.where(~self.pos, 0.0, np.where(self.nz, 1.0 - self.tt, 1.0)))
        be = np.where(~self.act, 0.0, np.where(
            ~self.pos, self.app, np.where(self.nz, self.app - (1.0 - self.tt) * self.ab, -self.ab)))
        self.al, self.be = affine_scan_inclusive(al, be)

    def check(self, c_in):
        """re-check against the input c_in; True if a branch changed"""
        v = affine_before(self.al, self.be, c_in) - self.ab
        pos2 = np.ones(WAVE, bool) if self.sq else ~(v < 0)
        self.m = self.app - self.tt * np.where(pos2, v, 0.0)
        nz2 = self.m > 0
        bad = self.act & ((pos2 != self.pos) | (pos2 & (nz2 != self.nz)))
        self.pos, self.nz = pos2, nz2
        if bad.any():
            self.first_bad.append(int(np.argmax(bad)))
        return bool(bad.any())

    def total(self):
        k = int(self.act.sum())
        return (self.al[k - 1], self.be[k - 1]) if k else (1.0, 0.0)


def emulate_lanes_deg2(case):
    """rounds of the one-wave scan loop (scans evaluated), lanes of each round's first mismatch"""
    w = _Deg2Wave(case, 0)
    c0 = float(case["cache_in"][0 if w.sq else 1])
    w.pos = np.ones(WAVE, bool) if w.sq else (c0 - w.ab) >= 0
    w.nz = (w.app - w.tt * np.where(w.pos, c0 - w.ab, 0.0)) > 0
    rounds = 0
    for _ in range(WAVE + 1):
        w.scan()
        rounds += 1
        if not w.check(c0):
            return dict(rounds=rounds, first_bad=w.first_bad, converged=True, zero=~(w.m > 0))
    return dict(rounds=rounds, first_bad=w.first_bad, converged=False, zero=~(w.m > 0))


def emulate_waves(case):
    """wave-level repeats of the wide chain and which waves changed a branch in each"""
    n = len(case["p_old"])
    sq = case["reg"] == "squaredl12"
    c0 = float(case["cache_in"][0 if sq else 1])
    waves = [_Deg2Wave(case, 64 * w) for w in range(8)]
    for w in waves:
        w.guess(c0)
    maps = [w.total() for w in waves]
    changed_log, local_max = [], 0
    for gr in range(3 * WAVE):
        new_maps, changed = list(maps), []
        for wi, w in enumerate(waves):
            c_in = c0
            for k in range(wi):
                c_in = maps[k][0] * c_in + maps[k][1]
            ch = False
            for lr in range(WAVE + 1):
                if not w.check(c_in):
                    break
                ch = True
                w.scan()
                local_max = max(local_max, lr + 1)
            if ch:
                new_maps[wi] = w.total()
                changed.append(wi)
        maps = new_maps
        changed_log.append(changed)
        if not changed:
            break
    zero = np.concatenate([~(w.m > 0) | ~w.act for w in waves])[:n]
    return dict(repeats=len(changed_log), changed=changed_log, local_max=local_max, zero=zero,
                converged=not changed_log[-1])


def _prefix_before(v, c0):
    inc = affine_scan_inclusive(np.ones(WAVE), v)[1]
    return c0 + np.concatenate(([0.0], inc[:-1]))


def emulate_deg3(case):
    """the guessed-r fixed point of degree-3 omegati: rounds run, and the path -- 'fixed' (the
    parallel result is taken) or 'serial' (a negative dc, or no fixed point in 8 rounds)"""
    a, p, s, act = _lane_constants(case)
    c10, c20 = float(case["cache_in"][1]), float(case["cache_in"][2])
    r = np.maximum(p - s * (c20 - (c10 - a) * a), 0.0)
    fixed, neg, rounds = False, False, 0
    while rounds < 8 and not fixed:
        d1 = r - a
        dc2 = _prefix_before(d1, c10) - a
        dc3 = _prefix_before(dc2 * d1, c20) - dc2 * a
        rn = np.maximum(p - s * dc3, 0.0)
        neg = bool((act & (np.signbit(dc2) | np.signbit(dc3))).any())
        fixed = bool((rn == r).all())
        r = rn
        rounds += 1
    return dict(rounds=rounds, path="fixed" if (fixed and not neg) else "serial",
                why=("ok" if fixed and not neg else ("clip" if neg else "cap")))


# ------------------------------------------------------------------ cases
def _esp(values, degree):
    c = np.zeros(degree + 1)
    c[0] = 1.0
    for v in values:
        for t in range(degree, 0, -1):
            c[t] += c[t - 1] * v
    return c


def _cache_for(reg, degree, abs_p, others):
    """the cache in front of column 0: sums over the step's columns and the row's other columns"""
    allv = np.concatenate((abs_p, others))
    if reg == "squaredl12":
        return np.array([allv.sum(), 0.0, 0.0])
    if degree == 0:
        return np.array([np.prod(1.0 + allv)])
    return _esp(allv, degree)


def _mk(cid, form, reg, degree, p_old, g, h, cache_in, lam=1.0, mu=1.0, beta=0.1, gamma=0.3,
        eta=1.0, **tags):
    case = dict(id=cid, form=form, reg=reg, degree=degree, lam=lam, mu=mu, beta=beta, gamma=gamma,
                eta=eta, p_old=np.asarray(p_old, dtype=np.float64),
                g=np.asarray(g, dtype=np.float64), h=np.asarray(h, dtype=np.float64),
                cache_in=np.asarray(cache_in, dtype=np.float64), generic=True, exact=False)
    case.update(tags)
    return case


def _random(cid, form, reg, degree, ncols, seed, gamma=0.3, beta=0.1, zero_frac=0.2, clip_at=None,
            accept=None, n_others=8, **tags):
    """A random step whose exact chain keeps the margin at every decision (acceptance loop).
    clip_at: columns whose |p_old| the cache under-states, which forces the clip there."""
    for attempt in range(200):
        rng = np.random.RandomState(1000 * seed + attempt)
        p = 0.5 * rng.randn(ncols)
        p[rng.rand(ncols) < zero_frac] = 0.0
        g = rng.randn(ncols) * 0.5
        h = rng.uniform(0.5, 2.0, ncols)
        others = np.abs(0.5 * rng.randn(n_others)) + 0.05   # 8: more than any degree, no e_t is 0
        table = np.abs(p).copy()
        if clip_at is not None:
            for j in clip_at:
                p[j] = 40.0 * (1.0 if rng.rand() < 0.5 else -1.0)
                table[j] = 0.125
        case = _mk(cid, form, reg, degree, p, g, h, _cache_for(reg, degree, table, others),
                   gamma=gamma, beta=beta, **tags)
        ex = exact_chain(case)
        if margin(case, ex) < CLEAR:
            continue
        if accept is not None and not accept(case, ex):
            continue
        return case
    raise AssertionError("no acceptable draw for %s" % cid)


def _dump_decay(cid, form, reg, ncols, start, a=0.001, big=1.9, others_c=0.01, **tags):
    """Many re-check rounds: columns in front of `start` are empty; column `start` lifts the cache
    from others_c to ~big, which sends every later column to zero -- but the guess (all columns at
    the initial cache) has them non-zero, and with 1 - t = 0.01 the guessed maps forget the lift
    within two columns: every round repairs about two more lanes."""
    t = 0.99
    st = t if reg == "omegati" else t / (2.0 * (1.0 - t))       # squaredl12: tt = 2 st/(1 + 2 st)
    den = 1.0 if reg == "omegati" else 1.0 + 2.0 * st
    p = np.zeros(ncols)
    pin = np.zeros(ncols)
    p[start + 1:] = a * np.where(np.arange(ncols - start - 1) % 2 == 0, 1.0, -1.0)
    pin[start] = big * den / t
    pin[start + 1:] = den * np.where(np.arange(ncols - start - 1) % 3 == 0, -1.0, 1.0)
    # beta = 0, h = mu = lam = eta = 1: p_in = p_old - g, strength = gamma
    cache = np.array([others_c + np.abs(p).sum(), 0.0, 0.0])
    if reg == "omegati":
        cache = np.array([1.0, cache[0], 0.0])
    return _mk(cid, form, reg, 2, p, p - pin, np.ones(ncols), cache, beta=0.0, gamma=st, **tags)


def _clip_scan(cid, form, ncols, seed):
    """degree-2 omegati with the al = 0 map inside the scan: column 10's clip appears only once the
    cache has fallen (the guess at the initial cache misses it), column 20's is there from the
    start (the guess has it); the cache under-states both columns."""
    for attempt in range(200):
        c = _clip_scan_draw(cid, form, ncols, 100 * seed + attempt)
        if margin(c, exact_chain(c)) >= CLEAR:
            return c
    raise AssertionError("no acceptable draw for %s" % cid)


def _clip_scan_draw(cid, form, ncols, seed):
    rng = np.random.RandomState(seed)
    p = 0.3 * np.where(rng.rand(ncols) < 0.5, 1.0, -1.0)
    pin = 0.2 * rng.randn(ncols)
    p[10], p[20] = 3.0, -50.0
    pin[10], pin[20] = 1.5, -2.5
    pin[30:] = 4.0 * np.where(rng.rand(ncols - 30) < 0.5, 1.0, -1.0)
    cache = np.array([1.0, 5.0, 0.0])
    return _mk(cid, form, "omegati", 2, p, p - pin, np.ones(ncols), cache, beta=0.0, gamma=0.4,
               clip_cols=(10, 20), generic=True)


def _tie(cid, form, reg, degree, ncols, seed):
    """Small dyadic numbers, h mu + beta = 1, eta = 1, strength 1/2: every intermediate of every
    form is exact in float64, and some m is exactly 0."""
    for attempt in range(4000):
        rng = np.random.RandomState(7000 * seed + attempt)
        q = 8.0 if degree <= 2 else 2.0
        p = rng.randint(-8, 9, ncols) / q
        g = rng.randint(-8, 9, ncols) / q
        if degree == 0:
            p = rng.choice([0.0, 0.0, 0.0, 1.0, -1.0], ncols)
        others = rng.randint(0, 5, 2) / q if degree else np.array([0.0])
        case = _mk(cid, form, reg, degree, p, g, np.full(ncols, 0.5),
                   _cache_for(reg, degree, np.abs(p), others), beta=0.5, gamma=0.5,
                   generic=False, exact=True)
        ex = exact_chain(case)
        ms = [d["m"] for d in ex["dec"]]
        if any(m == 0 for m in ms) and any(m > 0 for m in ms) and not ex["clipped"]:
            return case
    raise AssertionError("no tie found for %s" % cid)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = out.append
    # -- column counts on the DPP row boundaries, branch pattern changing across them (random)
    for n in LANES_NCOLS:
        add(_random("l1-n%d" % n, 0, "l1", 2, n, 1))
        add(_random("sq-n%d" % n, 0, "squaredl12", 2, n, 2, gamma=0.2))
        add(_random("ti2-n%d" % n, 0, "omegati", 2, n, 3))
    for n in WAVES_NCOLS:
        add(_random("w-sq-n%d" % n, 1, "squaredl12", 2, n, 4, gamma=0.4 / n))
        add(_random("w-ti2-n%d" % n, 1, "omegati", 2, n, 5, gamma=0.8 / n))
    add(_random("w-l1-n449", 1, "l1", 2, 449, 6))
    # -- many rounds; the first mismatch in each DPP row
    for reg, tag in (("squaredl12", "sq"), ("omegati", "ti2")):
        for start in (0, 15, 31, 47):
            c = _dump_decay("%s-rounds-s%d" % (tag, start), 0, reg, 64, start, want_row=(start + 1) // 16)
            c["id"] += "-r%d" % emulate_lanes_deg2(c)["rounds"]
            add(c)
        add(_dump_decay("w-%s-repeats" % tag, 1, reg, 512, 0, a=0.0005, want_repeats=3))
    # -- wide: waves 2-6 empty; only the last wave's branches change
    for reg, tag in (("squaredl12", "sq"), ("omegati", "ti2")):
        c = _random("w-%s-mid-empty" % tag, 1, reg, 2, 512, 8, gamma=0.004)
        c["p_old"][128:448] = 0.0
        c["g"][128:448] = 0.0
        c["mid_empty"] = True
        assert margin(c, exact_chain(c)) >= CLEAR
        add(c)
        n = 512
        p = np.full(n, 0.01)
        pin = np.zeros(n)
        pin[448:] = 3.0
        st = 0.5
        den = 1.0 if reg == "omegati" else 1.0 + 2.0 * st
        cache = np.array([8.0, 0.0, 0.0]) if reg == "squaredl12" else np.array([1.0, 8.0, 0.0])
        add(_mk("w-%s-last-wave" % tag, 1, reg, 2, p, p - pin * den, np.ones(n), cache, beta=0.0,
                gamma=st, last_wave_only=True))
    # -- the al = 0 clip map inside the scan
    add(_clip_scan("ti2-clip-scan-n64", 0, 64, 1))
    add(_clip_scan("ti2-clip-scan-n33", 0, 33, 2))
    add(_clip_scan("w-ti2-clip-scan-n200", 1, 200, 3))
    # -- degree 3: strengths 0.1 - 1
    add(_random("ti3-fixed", 0, "omegati", 3, 37, 11, gamma=0.25, want_path="fixed",
                accept=lambda c, ex: emulate_deg3(c)["why"] == "ok"
                and 3 <= emulate_deg3(c)["rounds"] <= 7))
    add(_random("ti3-cap", 0, "omegati", 3, 64, 12, gamma=0.1, n_others=3, want_path="cap",
                accept=lambda c, ex: emulate_deg3(c)["why"] == "cap"))
    add(_random("ti3-clip", 0, "omegati", 3, 37, 13, gamma=0.25, clip_at=(9,), want_path="clip",
                accept=lambda c, ex: ex["clipped"]))
    for n in LANES_NCOLS:
        add(_random("ti3-n%d" % n, 0, "omegati", 3, n, 14, gamma=0.2,
                    accept=lambda c, ex: not ex["clipped"]))
    # -- degrees 4-6 and all-subsets: the serial loop, its block tail, clips by position
    for M in (4, 5, 6, 0):
        for last in SERIAL_LAST:
            add(_random("ti%d-last%d" % (M, last), 0, "omegati", M, last + 1, 20 + M,
                        gamma=0.2 if M else 0.05, accept=lambda c, ex: not ex["clipped"]))
    for M in (4, 5, 6):
        n = 23
        for where, j in (("first", 0), ("last", n - 1), ("blk3", 3), ("blk4", 4)):
            add(_random("ti%d-clip-%s" % (M, where), 0, "omegati", M, n, 30 + M, gamma=0.2,
                        clip_at=(j,), clip_col=j,
                        accept=lambda c, ex, j=j: all(v >= 0 for d in ex["dec"][:j] for v in d["v"])
                        and ex["dec"][j]["v"][0] < 0))
    # -- degenerate inputs
    for reg, M, tag in (("l1", 2, "l1"), ("squaredl12", 2, "sq"), ("omegati", 2, "ti2"),
                        ("omegati", 3, "ti3"), ("omegati", 5, "ti5"), ("omegati", 0, "tias")):
        n = 37
        c = _random("%s-pold0" % tag, 0, reg, M, n, 40, zero_frac=1.1)
        assert not c["p_old"].any()
        add(c)
        add(_random("%s-gamma0" % tag, 0, reg, M, n, 41, gamma=0.0, none_zero=True))
        c = _random("%s-h0" % tag, 0, reg, M, n, 42, beta=0.7)
        c["h"][:] = 0.0
        assert margin(c, exact_chain(c)) >= CLEAR
        add(c)
        add(_random("%s-all-zero" % tag, 0, reg, M, n, 43, gamma=60.0, all_zero=True))
        if reg != "l1":
            c = _random("%s-cache0" % tag, 0, reg, M, n, 44, zero_frac=1.1)
            c["cache_in"] = np.zeros_like(c["cache_in"])
            if M == 0:
                c["cache_in"][0] = 1.0     # the empty product
            if M != 0 and reg == "omegati":
                c["cache_in"][0] = 1.0
            c["generic"] = reg == "squaredl12" or M == 0   # omegati: every clip argument is 0
            add(c)
    # -- exact ties
    add(_tie("tie-l1", 0, "l1", 2, 33, 1))
    add(_tie("tie-sq", 0, "squaredl12", 2, 33, 2))
    add(_tie("tie-ti2", 0, "omegati", 2, 33, 3))
    add(_tie("w-tie-sq", 1, "squaredl12", 2, 33, 4))
    add(_tie("w-tie-ti2", 1, "omegati", 2, 33, 5))
    add(_tie("tie-ti3", 0, "omegati", 3, 5, 6))
    add(_tie("tie-ti4", 0, "omegati", 4, 5, 7))
    add(_tie("tie-tias", 0, "omegati", 0, 6, 8))
    # -- forms 0 and 1 on the same input (ncols <= 64, degree 2)
    for c in [c for c in out if c["form"] == 0 and c["degree"] == 2]:
        if c["id"].split("-")[0] in ("sq", "ti2") and ("rounds" in c["id"] or "clip" in c["id"]
                                                        or c["id"].endswith(("n17", "n64"))):
            twin = dict(c, id="w=" + c["id"], form=1, twin_of=c["id"])
            out.append(twin)
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exact_of(cid):
    return exact_chain(case_by_id(cid))


def case_by_id(cid):
    return next(c for c in cases() if c["id"] == cid)


def case_ids():
    return [c["id"] for c in cases()]


# ------------------------------------------------------------------ tests (no GPU)
def test_exact_reference_against_host_face():
    """exact_chain against the project's float64 regularizer objects driven column by column as
    pcd.py drives them (they are replayed against reference traces elsewhere)."""
    from sparsepoly_amd.regularizer import L1, OmegaTI, SquaredL12

    for cid in ("l1-n33", "sq-n33", "ti2-n33", "ti3-n33", "ti5-last7", "ti0-last62",
                "ti4-clip-blk3", "ti2-clip-scan-n33"):
        case = case_by_id(cid)
        ex = exact_of(cid)
        reg = {"l1": L1, "squaredl12": SquaredL12, "omegati": OmegaTI}[case["reg"]]()
        n, M = len(case["p_old"]), case["degree"]
        deg = -1 if M == 0 else M
        reg.init_cache_pcd(deg, n, 1)
        P = case["p_old"].copy()[None, :]
        if case["reg"] != "l1":
            reg._abs_p[:] = np.abs(P[0])
            if M == 0:
                reg._cache_all_subsets = float(case["cache_in"][0])
            elif case["reg"] == "squaredl12":
                reg._cache[0] = case["cache_in"][0]
            else:
                reg._cache[:] = case["cache_in"]
                reg._dcache[:] = 0.0
                reg._dcache[1] = 1.0
        for j in range(n):
            inv = case["h"][j] * case["mu"] + case["beta"]
            upd = (case["g"][j] * case["lam"] + case["beta"] * P[0, j]) / inv
            P[0, j] = reg.prox_cd(P[0, j] - case["eta"] * upd, case["eta"] * case["gamma"] / inv,
                                  deg, j)
            reg.update_cache_pcd(P, deg, 0, j)
        want = np.array([float(v) for v in ex["p"]])
        tol = 1e-12 * ex["scale"]
        np.testing.assert_allclose(P[0], want, rtol=0, atol=tol, err_msg=cid)
        assert ((P[0] == 0) == (want == 0)).all(), cid
        fl, _ = float_chain(case)
        np.testing.assert_allclose(fl, want, rtol=0, atol=tol, err_msg=cid)


def test_column_counts():
    cs = cases()
    for reg, M in (("l1", 2), ("squaredl12", 2), ("omegati", 2), ("omegati", 3)):
        have = {len(c["p_old"]) for c in cs if c["form"] == 0 and c["reg"] == reg
                and c["degree"] == M}
        assert set(LANES_NCOLS) <= have, (reg, M)
    for M in (4, 5, 6, 0):
        have = {len(c["p_old"]) - 1 for c in cs if c["form"] == 0 and c["degree"] == M
                and c["reg"] == "omegati"}
        assert set(SERIAL_LAST) <= have, M
    for reg in ("squaredl12", "omegati"):
        have = {len(c["p_old"]) for c in cs if c["form"] == 1 and c["reg"] == reg}
        assert set(WAVES_NCOLS) <= have, reg


def test_margins_and_scan_contraction():
    """every generic case: each decision clear of its threshold; degree-2 scans: |al| <= 1 in the
    maps of the final (true) branches, which the derived bound of the GPU file relies on"""
    for c in cases():
        ex = exact_of(c["id"])
        if c["generic"]:
            assert margin(c, ex) >= CLEAR, c["id"]
        if c["degree"] == 2 and c["reg"] != "l1":
            _, _, tt, _ = _lane_constants(c, 0, len(c["p_old"]))
            nzc = np.array([v != 0 for v in ex["p"]])      # the maps x -> (1 - tt)(x - a) + p
            assert (tt >= 0).all() and (tt[nzc] <= 1).all(), c["id"]


def test_round_counts_and_paths():
    by = {c["id"]: c for c in cases()}
    rows = {"sq": set(), "ti2": set()}
    for cid, c in by.items():
        if "-rounds-" in cid and c["form"] == 0:
            e = emulate_lanes_deg2(c)
            assert e["converged"] and e["rounds"] >= (16 if "-s0-" in cid else 2), (cid, e["rounds"])
            assert cid.endswith("-r%d" % e["rounds"])
            assert e["first_bad"][0] // 16 == c["want_row"], (cid, e["first_bad"][:3])
            rows[cid.split("-")[0]].add(e["first_bad"][0] // 16)
        if c.get("want_repeats"):
            e = emulate_waves(c)
            assert e["converged"] and e["repeats"] >= c["want_repeats"], (cid, e["repeats"])
            assert e["local_max"] <= WAVE
        if c.get("mid_empty"):
            ex = exact_of(cid)
            assert not c["p_old"][128:448].any() and not any(ex["p"][128:448])
            assert any(ex["p"][:128]) and any(ex["p"][448:])
        if c.get("last_wave_only"):
            e = emulate_waves(c)
            assert e["converged"] and e["changed"][0] == [7], (cid, e["changed"])
        if c.get("want_path"):
            e = emulate_deg3(c)
            assert e["why"] == {"fixed": "ok", "cap": "cap", "clip": "clip"}[c["want_path"]], (cid, e)
            if c["want_path"] == "fixed":
                assert 3 <= e["rounds"] <= 7, (cid, e)
            if c["want_path"] == "cap":
                assert e["rounds"] == 8
    assert rows == {"sq": {0, 1, 2, 3}, "ti2": {0, 1, 2, 3}}, rows


def test_emulation_predicts_the_exact_branches():
    """the emulated schemes end at the exact reference's zero set (they are fixed-point forms of
    the same chain) on every degree-2 case"""
    for c in cases():
        if c["degree"] != 2 or c["reg"] == "l1" or c["exact"]:
            continue
        ex = exact_of(c["id"])
        want = np.array([v == 0 for v in ex["p"]])
        e = emulate_waves(c) if c["form"] == 1 else emulate_lanes_deg2(c)
        got = e["zero"][:len(want)]
        assert e["converged"] and (got == want).all(), c["id"]


def test_clip_cases():
    by = {c["id"]: c for c in cases()}
    for cid in ("ti2-clip-scan-n64", "ti2-clip-scan-n33", "w-ti2-clip-scan-n200"):
        c, ex = by[cid], exact_of(cid)
        ab = np.abs(c["p_old"])
        c0 = c["cache_in"][1]
        assert ex["dec"][10]["v"][0] < 0 and c0 - ab[10] >= 0     # the guess misses this clip
        assert ex["dec"][20]["v"][0] < 0 and c0 - ab[20] < 0      # the guess has this one
        assert sum(d["v"][0] < 0 for d in ex["dec"]) < len(ab) // 2
    for cid, c in by.items():
        if "clip_col" in c:
            assert exact_of(cid)["dec"][c["clip_col"]]["v"][0] < 0, cid
        if cid.startswith("ti") and "-last" in cid and "clip" not in cid:
            assert not exact_of(cid)["clipped"], cid


def test_degenerate_and_tie_cases():
    for c in cases():
        ex = exact_of(c["id"])
        if c.get("all_zero"):
            assert not any(ex["p"]), c["id"]
        if c.get("none_zero"):
            assert all(v != 0 for v, pin in zip(ex["p"], c["p_old"])) or c["reg"] == "l1", c["id"]
        if c["exact"]:
            ms = [d["m"] for d in ex["dec"]]
            assert any(m == 0 for m in ms) and (c["h"] * c["mu"] + c["beta"] == 1.0).all()
            assert c["eta"] == 1.0
            # every exact value is a float64
            assert all(Fr(float(v)) == v for v in ex["p"]) and all(Fr(float(v)) == v for v in ex["cache"])


def test_baseline_error_within_derived_bound():
    """plain sequential float64 against the exact chain: inside the running bound that the GPU
    file asserts for the device (without that file's scan and association terms)"""
    worst = 0.0
    for c in cases():
        ex = exact_of(c["id"])
        fl, fc = float_chain(c)
        want = np.array([float(v) for v in ex["p"]])
        bound = U * (2.0 * ex["err_p"] + ex["scale"])
        ratio = np.abs(fl - want) / bound
        assert (ratio <= 1.0).all(), (c["id"], ratio.max())
        worst = max(worst, float(ratio.max()))
    print("baseline error / bound, worst: %.3f" % worst)
