#!/usr/bin/env python3
"""Timing of one epoch of the pairwise ranking fit with its negatives drawn on the device by the
WARP sampler (``spfm_psgd_pairs_sample_warp``) beside the uniform and the
hardest-of-M samplers of section 19a, each followed by ``spfm_psgd_pairs_epoch_sampled``.  The
shape and the protocol are those of ``tools/bench_pairwise_sample.py``: same build, same process,
one handle per route on the same data and parameters, the routes interleaved; warm-up epochs
first, then the median of ``--runs`` epochs each (host clock around calls that end in a device
synchronise).  The sample call is timed on its own as well, and after the timed epochs the share
of zero-weight triples of one more WARP draw at the parameters then live is recorded.  One WARP
route per value of ``--margins``.  Not the driver benchmark (bench.py).

``--guard OTHER.json``: compare ``pair_epoch_ms`` of two ``tools/bench_pairwise.py`` results
(this build's first, the parent build's second, run one after the other in one session): this
build's median may exceed the parent's by no more than the larger of the two runs' ranges.

``--quality``: also fit the planted two-tower problem of the tests for 10 epochs with each
sampler from one seed and record ``recall@10`` of ``rank_metrics`` on the held-out interactions
(an observation, not a claim)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def guard(mine, parent):
    """the run-order guard on two bench_pairwise.py results"""
    a, b = (json.load(open(p)) for p in (mine, parent))
    ra = max(a["pair_epoch_ms_all"]) - min(a["pair_epoch_ms_all"])
    rb = max(b["pair_epoch_ms_all"]) - min(b["pair_epoch_ms_all"])
    out = dict(tool="bench_pairwise_warp --guard", this_build=a["build_tag"],
               parent_build=b["build_tag"], this_pair_epoch_ms=a["pair_epoch_ms"],
               parent_pair_epoch_ms=b["pair_epoch_ms"], this_all=a["pair_epoch_ms_all"],
               parent_all=b["pair_epoch_ms_all"], this_range_ms=round(ra, 3),
               parent_range_ms=round(rb, 3),
               excess_ms=round(a["pair_epoch_ms"] - b["pair_epoch_ms"], 3),
               allowed_ms=round(max(ra, rb), 3))
    out["ok"] = bool(out["excess_ms"] <= out["allowed_ms"])
    print(json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


def quality(n_candidates, margin):
    from bench_pairwise_sample import planted_problem
    from sparsepoly_amd import SparseFactorizationMachineRanker

    X, Z, train, held = planted_problem()
    out = {}
    for sampler in ("uniform", "dynamic", "warp"):
        est = SparseFactorizationMachineRanker(
            degree=2, n_components=6, fit_lower=None, regularizer="l1", alpha=1e-3, beta=1e-2,
            gamma=1e-4, eta0=0.5, learning_rate="invscaling", power_t=0.3, batch_size=64,
            max_iter=10, tol=-1.0, n_iter_no_change=1000, shuffle=True, random_state=3,
            precision="f64")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est.fit(X, Z, interactions=train, n_negatives=2, sampler=sampler,
                    n_candidates=n_candidates, margin=margin)
        got = est.rank_metrics(X, Z, held, exclude=train, ks=(10,))
        out[sampler] = round(float(got["recall@10"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--contexts", type=int, default=100_000)
    ap.add_argument("--candidates", type=int, default=20_000)
    ap.add_argument("--ctx-features", type=int, default=50_000)
    ap.add_argument("--positives", type=int, default=400_000)
    ap.add_argument("--batch", type=int, default=4096, help="triples per minibatch")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--candidates-per-draw", type=int, default=8)
    ap.add_argument("--margins", default="1.0,0.0", help="one WARP route per margin")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--guard", nargs=2, metavar=("THIS.json", "PARENT.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"),
                    help="directory of pairwise_warp_<build tag>.json")
    a = ap.parse_args()
    if a.guard:
        return guard(*a.guard)

    from bench_pairwise import build_sides
    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    B, C, k, M = a.contexts, a.candidates, a.k, a.candidates_per_draw
    margins = [float(v) for v in a.margins.split(",")]
    X, Z = build_sides(B, C, a.ctx_features, a.seed)
    d = X.shape[1]
    rng = np.random.RandomState(a.seed + 2)
    I = sp.csr_matrix((np.ones(a.positives),
                       (rng.randint(0, B, a.positives), rng.randint(0, C, a.positives))),
                      shape=(B, C))
    I.sum_duplicates()
    I.sort_indices()
    I.data[:] = 1.0
    m = int(I.nnz)
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    P0 = 0.01 * np.random.RandomState(a.seed + 3).randn(1, k, d)
    hyper = (2, 1e-3, 1e-3, 1e-4, 0.05, "optimal", 1.0)
    routes = ["uniform", "dynamic"] + ["warp_margin_%g" % mg for mg in margins]
    margin_of = dict(zip(routes[2:], margins))
    eng = {}
    for route in routes:
        e = HipEngine(0, "f32")
        e.set_data(S, np.zeros(B + C))
        e.set_params(P0, np.zeros(d), np.ones(k))
        e.configure("psgd", "logistic", "l1", 2)
        e.psgd_pairs_set_sampler(B, C, I)
        eng[route] = e
    it = {r: 1 for r in eng}

    def run(route, ep):
        e = eng[route]
        t0 = time.perf_counter()
        if route in margin_of:
            e.psgd_pairs_sample_warp(2, 1, M, 64 * M, margin_of[route], 12345, ep, None,
                                     want=False)
        else:
            mc = 1 if route == "uniform" else M
            e.psgd_pairs_sample(2, 1, mc, 64 * mc, 12345, ep, None, want_triples=False,
                                want_scores=False)
        t1 = time.perf_counter()
        sl, it[route] = e.psgd_pairs_epoch_sampled(*hyper, a.batch, True, it[route])
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, sl / m

    total = {r: [] for r in eng}
    draw = {r: [] for r in eng}
    loss = {}
    for ep in range(a.warmup + a.runs):  # interleaved: drift of the machine hits all alike
        for route in routes:
            dt, ds, loss[route] = run(route, ep)
            if ep >= a.warmup:
                total[route].append(dt)
                draw[route].append(ds)
    assert len(set(it.values())) == 1
    zero, trials = {}, {}
    for route in margin_of:  # one more draw, not timed, at the parameters the route ended with
        _, _, _, wt, tr = eng[route].psgd_pairs_sample_warp(2, 1, M, 64 * M, margin_of[route],
                                                            12345, a.warmup + a.runs)
        zero[route] = round(float((wt == 0).mean()), 4)
        trials[route] = dict(none=round(float((tr == 0).mean()), 4),
                             first=round(float((tr == 1).mean()), 4),
                             mean_when_found=round(float(tr[tr > 0].mean()), 3) if (tr > 0).any()
                             else None)

    def ms(v):
        return dict(median=round(float(np.median(v)) * 1e3, 3), lo=round(min(v) * 1e3, 3),
                    hi=round(max(v) * 1e3, 3), all=[round(x * 1e3, 3) for x in v])

    tag = _capi.load().spfm_build_tag().decode()
    out = dict(
        tool="bench_pairwise_warp", build_tag=tag, device=eng["uniform"].device_name,
        contexts=B, candidates=C, features=d, k=k, positives=m, n_negatives=1, batch_size=a.batch,
        updates_per_epoch=-(-m // a.batch), n_candidates=M, max_draws=64 * M, warmup=a.warmup,
        runs=a.runs,
        epoch_ms={r: ms(total[r]) for r in eng},
        draw_ms={r: ms(draw[r]) for r in eng},
        draw_share={r: round(float(np.median(draw[r]) / np.median(total[r])), 4) for r in eng},
        mean_weighted_loss_last_epoch={r: round(loss[r], 6) for r in eng},
        zero_weight_share_after_the_timed_epochs=zero,
        trials_after_the_timed_epochs=trials,
        timing="host clock; epoch_ms: drawing the negatives plus the epoch call, which ends in a "
               "device synchronise; draw_ms: the sample call alone (one kernel and a synchronise)")
    if a.quality:
        out["planted_recall_at_10_after_10_epochs"] = quality(M, margins[0])
        out["planted_margin"] = margins[0]
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "pairwise_warp_%s.json" % tag)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    for e in eng.values():
        e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
