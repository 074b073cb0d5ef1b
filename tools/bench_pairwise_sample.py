#!/usr/bin/env python3
"""Timing of one epoch of the pairwise ranking fit with its negatives drawn (a) on the host, as
before -- ``sample_triples``, the 12 m byte upload, ``spfm_psgd_pairs_epoch`` with its host check
--, (b) on the device, uniformly (``spfm_psgd_pairs_sample`` with one candidate, then
``spfm_psgd_pairs_epoch_sampled``) and (c) on the device, hardest of ``--candidates-per-draw``
(DESIGN.md section 19a).  Same build, same process, three handles on the same data and
parameters, the routes interleaved; warm-up epochs first, then the median of ``--runs`` epochs
each (host clock around calls that end in a device synchronise).  The sample call of (b) and (c)
is timed on its own as well.  Not the driver benchmark (bench.py).

The shape is that of ``tools/bench_pairwise.py``: contexts of about 30 stored entries, candidates
of one to three, k = 30, degree 2, l1, logistic loss, f32 storage.

``--quality``: also fit the planted two-tower problem of the tests for 10 epochs with
``sampler='uniform'`` and ``sampler='dynamic'`` from one seed and record ``recall@10`` of
``rank_metrics`` on the held-out interactions (an observation, not a claim)."""
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
from bench_pairwise import build_sides  # noqa: E402
from sparsepoly_amd import SparseFactorizationMachineRanker, _capi, sample_triples  # noqa: E402
from sparsepoly_amd.engine import HipEngine  # noqa: E402


def planted_problem():
    """200 contexts (a user id and two of eight attributes), 60 candidates (an item id); per
    context the four best candidates of a planted two-tower model train, the next two are held
    out"""
    rng = np.random.RandomState(7)
    B, Cn, r = 200, 60, 4
    order = np.argsort(-(rng.randn(B, r) @ rng.randn(Cn, r).T), axis=1)
    train = sp.csr_matrix((np.ones(B * 4), (np.repeat(np.arange(B), 4), order[:, :4].ravel())),
                          shape=(B, Cn))
    held = sp.csr_matrix((np.ones(B * 2), (np.repeat(np.arange(B), 2), order[:, 4:6].ravel())),
                         shape=(B, Cn))
    d = B + 8 + Cn
    attr = np.stack([rng.choice(8, 2, replace=False) for _ in range(B)])
    X = sp.csr_matrix((np.ones(3 * B),
                       (np.repeat(np.arange(B), 3),
                        np.column_stack([np.arange(B), B + attr]).ravel())), shape=(B, d))
    Z = sp.csr_matrix((np.ones(Cn), (np.arange(Cn), B + 8 + np.arange(Cn))), shape=(Cn, d))
    return X, Z, train, held


def quality(n_candidates):
    X, Z, train, held = planted_problem()
    out = {}
    for sampler in ("uniform", "dynamic"):
        est = SparseFactorizationMachineRanker(
            degree=2, n_components=6, fit_lower=None, regularizer="l1", alpha=1e-3, beta=1e-2,
            gamma=1e-4, eta0=0.5, learning_rate="invscaling", power_t=0.3, batch_size=64,
            max_iter=10, tol=-1.0, n_iter_no_change=1000, shuffle=True, random_state=3,
            precision="f64")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            est.fit(X, Z, interactions=train, n_negatives=2, sampler=sampler,
                    n_candidates=n_candidates)
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"),
                    help="directory of pairwise_sample_<build tag>.json")
    a = ap.parse_args()

    B, C, k, M = a.contexts, a.candidates, a.k, a.candidates_per_draw
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
    eng = {}
    for route in ("host", "uniform", "dynamic"):
        e = HipEngine(0, "f32")
        e.set_data(S, np.zeros(B + C))
        e.set_params(P0, np.zeros(d), np.ones(k))
        e.configure("psgd", "logistic", "l1", 2)
        if route != "host":
            e.psgd_pairs_set_sampler(B, C, I)
        eng[route] = e
    it = {r: 1 for r in eng}
    draw_rng = np.random.RandomState(a.seed + 4)
    shift = np.array([0, B, B], dtype=np.int32)

    def run_host(ep):
        t0 = time.perf_counter()
        t = sample_triples(I, 1, draw_rng)
        t1 = time.perf_counter()
        sl, it["host"] = eng["host"].psgd_pairs_epoch(*hyper, a.batch, t + shift, True, it["host"])
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, sl / m

    def run_device(route, ep):
        e = eng[route]
        t0 = time.perf_counter()
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
        for route in ("host", "uniform", "dynamic"):
            dt, ds, loss[route] = run_host(ep) if route == "host" else run_device(route, ep)
            if ep >= a.warmup:
                total[route].append(dt)
                draw[route].append(ds)
    assert it["host"] == it["uniform"] == it["dynamic"]

    def ms(v):
        return dict(median=round(float(np.median(v)) * 1e3, 3), lo=round(min(v) * 1e3, 3),
                    hi=round(max(v) * 1e3, 3), all=[round(x * 1e3, 3) for x in v])

    tag = _capi.load().spfm_build_tag().decode()
    out = dict(
        tool="bench_pairwise_sample", build_tag=tag, device=eng["host"].device_name,
        contexts=B, candidates=C, features=d, k=k, positives=m, n_negatives=1, batch_size=a.batch,
        updates_per_epoch=-(-m // a.batch), n_candidates=M, max_draws=64 * M, warmup=a.warmup,
        runs=a.runs,
        epoch_ms={r: ms(total[r]) for r in eng},
        draw_ms={r: ms(draw[r]) for r in eng},
        mean_loss_last_epoch={r: round(loss[r], 6) for r in eng},
        uploaded_bytes_per_triple=dict(host=12, uniform=0, dynamic=0),
        timing="host clock; epoch_ms: drawing the negatives plus the epoch call, which ends in a "
               "device synchronise; draw_ms: the drawing alone (host: sample_triples in NumPy; "
               "device: the sample call, one kernel and a synchronise)")
    if a.quality:
        out["planted_recall_at_10_after_10_epochs"] = quality(M)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "pairwise_sample_%s.json" % tag)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    for e in eng.values():
        e.close()


if __name__ == "__main__":
    main()
