#!/usr/bin/env python3
"""Timing of one epoch of the listwise ranking fit against the only
route the library offered before it for the same arithmetic: ``'list'`` over B lists per batch
is ``spfm_psgd_pairs_epoch`` over the same grouped triples with ``batch_size = B * M``.  The
``'softmax'`` epoch over the same lists is timed beside them.  Same build, same process, the
three routes interleaved; warm-up epochs first, then the median and the range of ``--runs``
epochs each (host clock around calls that end in a device synchronise; every route uploads the
same 12 m bytes of triples).  Not the driver benchmark (bench.py).

The shape is that of ``tools/bench_pairwise.py``: contexts of about 30 stored entries, candidates
of one to three, k = 30, degree 2, l1, logistic loss, an f32 handle.  Every value of
``--negatives`` runs over the same ``--positives`` positives, so a route's column shows how its
epoch grows with M.

``--profile-only``: warm-up and ``--runs`` epochs of the three routes at the first value of
``--negatives`` and nothing else, for a ``rocprofv3 --kernel-trace --stats`` run of this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_pairwise import build_sides  # noqa: E402
from sparsepoly_amd import _capi  # noqa: E402
from sparsepoly_amd.engine import HipEngine  # noqa: E402

HYPER = (2, 1e-3, 1e-3, 1e-4, 0.05, "optimal", 1.0)


def grouped_triples(B, C, Q, M, seed):
    """Q positives with M uniform negatives each (never the positive), grouped, rows of [X; Z]"""
    rng = np.random.RandomState(seed)
    b = rng.randint(0, B, Q)
    cp = rng.randint(0, C, Q)
    neg = (cp[:, None] + rng.randint(1, C, (Q, M))) % C
    t = np.stack([np.repeat(b, M), B + np.repeat(cp, M), B + neg.ravel()], axis=1)
    return np.ascontiguousarray(t, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--contexts", type=int, default=100_000)
    ap.add_argument("--candidates", type=int, default=20_000)
    ap.add_argument("--ctx-features", type=int, default=50_000)
    ap.add_argument("--positives", type=int, default=400_000)
    ap.add_argument("--negatives", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--batch", type=int, default=4096, help="lists per minibatch")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"),
                    help="directory of pairwise_list_<build tag>.json")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()

    B, C, Q, k = a.contexts, a.candidates, a.positives, a.k
    X, Z = build_sides(B, C, a.ctx_features, a.seed)
    d = X.shape[1]
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    P0 = 0.01 * np.random.RandomState(a.seed + 3).randn(1, k, d)
    routes = ("list", "pairs", "softmax")
    eng = {}
    for r in routes:
        eng[r] = HipEngine(0, "f32")
        eng[r].set_data(S, np.zeros(B + C))
        eng[r].set_params(P0, np.zeros(d), np.ones(k))
        eng[r].configure("psgd", "logistic", "l1", 2)

    rows = []
    for M in (a.negatives[:1] if a.profile_only else a.negatives):
        ts = grouped_triples(B, C, Q, M, a.seed + 2)
        it = {}
        for r in routes:
            eng[r].set_params(P0, np.zeros(d), np.ones(k))
            it[r] = 1

        def run(r):
            t0 = time.perf_counter()
            if r == "pairs":
                sl, it[r] = eng[r].psgd_pairs_epoch(*HYPER, a.batch * M, ts, True, it[r])
                sl /= M
            else:
                sl, it[r] = eng[r].psgd_lists_epoch(*HYPER, a.batch, ts, M, r, True, it[r])
            return time.perf_counter() - t0, sl / Q

        for _ in range(a.warmup):
            for r in routes:
                run(r)
        times = {r: [] for r in routes}
        losses = {}
        for _ in range(a.runs):  # interleaved: drift of the machine hits the routes alike
            for r in routes:
                dt, losses[r] = run(r)
                times[r].append(dt)
        assert it["list"] == it["pairs"] == it["softmax"]   # the same number of updates
        med = {r: float(np.median(v)) for r, v in times.items()}
        row = dict(n_negatives=M, triples=Q * M, updates_per_epoch=-(-Q // a.batch),
                   pairs_over_list=round(med["pairs"] / med["list"], 3),
                   mean_loss_last_epoch={r: round(losses[r], 6) for r in routes})
        for r in routes:
            row[r + "_epoch_ms"] = round(med[r] * 1e3, 3)
            row[r + "_epoch_ms_range"] = [round(min(times[r]) * 1e3, 3),
                                          round(max(times[r]) * 1e3, 3)]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.profile_only:
        return
    tag = _capi.load().spfm_build_tag().decode()
    out = dict(
        tool="bench_pairwise_list", build_tag=tag, device=eng["list"].device_name, contexts=B,
        candidates=C, features=d, k=k, positives=Q, lists_per_batch=a.batch, warmup=a.warmup,
        runs=a.runs, context_entries_mean=round(X.nnz / B, 2),
        candidate_entries_mean=round(Z.nnz / C, 2), by_n_negatives=rows,
        routes=dict(list="spfm_psgd_lists_epoch, SPFM_LIST_PAIRMEAN, batch_size lists",
                    pairs="spfm_psgd_pairs_epoch over the same grouped triples, batch_size * M "
                          "triples: the same arithmetic as 'list'",
                    softmax="spfm_psgd_lists_epoch, SPFM_LIST_SOFTMAX, batch_size lists"),
        timing="host clock around an epoch call that ends in a device synchronise; every route "
               "includes the upload of its 12 m bytes of triples; median and min .. max of the "
               "runs, routes interleaved")
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "pairwise_list_%s.json" % tag)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    for r in routes:
        eng[r].close()


if __name__ == "__main__":
    main()
