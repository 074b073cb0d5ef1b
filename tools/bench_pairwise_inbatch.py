#!/usr/bin/env python3
"""Timing of one epoch of the in-batch softmax against the route the
library offered before it for a softmax over negatives: ``spfm_psgd_lists_epoch`` with
``SPFM_LIST_SOFTMAX`` at ``--negatives`` sampled negatives per positive, on the same data and
the same positives.  Same build, same process, one handle per route, the routes interleaved;
warm-up epochs first, then the median and the range of ``--runs`` epochs each (host clock around
calls that end in a device synchronise; every route includes the upload of its pair or triple
list).  Not the driver benchmark (bench.py).

The shape and the protocol are those of ``tools/bench_pairwise_list.py``.  Besides ms per epoch
the table gives ms per epoch per negative seen by a positive: ``batch - 1`` for the in-batch
route (an upper bound: masked columns and the short last minibatch see fewer), M for a list.

``--profile-only``: warm-up and ``--runs`` epochs of the in-batch route alone, for a
``rocprofv3 --kernel-trace --stats`` run of this tool."""
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
from bench_pairwise_list import HYPER, grouped_triples  # noqa: E402
from sparsepoly_amd import _capi  # noqa: E402
from sparsepoly_amd.engine import HipEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--contexts", type=int, default=100_000)
    ap.add_argument("--candidates", type=int, default=20_000)
    ap.add_argument("--ctx-features", type=int, default=50_000)
    ap.add_argument("--positives", type=int, default=400_000)
    ap.add_argument("--negatives", type=int, nargs="+", default=[4, 16, 63])
    ap.add_argument("--batch", type=int, default=4096, help="positives per minibatch")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"),
                    help="directory of pairwise_inbatch_<build tag>.json")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()

    B, C, Q, k = a.contexts, a.candidates, a.positives, a.k
    X, Z = build_sides(B, C, a.ctx_features, a.seed)
    d = X.shape[1]
    S = sp.vstack([X, Z], format="csr")
    S.sort_indices()
    P0 = 0.01 * np.random.RandomState(a.seed + 3).randn(1, k, d)
    negs = [] if a.profile_only else list(a.negatives)
    # the lists of every M share their positives (grouped_triples draws them first)
    lists = {M: grouped_triples(B, C, Q, M, a.seed + 2) for M in negs}
    pairs = np.ascontiguousarray(grouped_triples(B, C, Q, 1, a.seed + 2)[:, :2])
    routes = ["in_batch"] + ["softmax_M%d" % M for M in negs]
    eng, it = {}, {}
    for r in routes:
        eng[r] = HipEngine(0, "f32")
        eng[r].set_data(S, np.zeros(B + C))
        eng[r].set_params(P0, np.zeros(d), np.ones(k))
        eng[r].configure("psgd", "logistic", "l1", 2)
        it[r] = 1

    def run(r):
        t0 = time.perf_counter()
        if r == "in_batch":
            sl, it[r] = eng[r].psgd_inbatch_epoch(*HYPER, a.batch, pairs, True, it[r])
        else:
            M = int(r.split("M")[1])
            sl, it[r] = eng[r].psgd_lists_epoch(*HYPER, a.batch, lists[M], M, "softmax", True,
                                                it[r])
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
    assert len(set(it.values())) == 1   # the same number of updates
    rows = []
    for r in routes:
        seen = a.batch - 1 if r == "in_batch" else int(r.split("M")[1])
        med = float(np.median(times[r]))
        rows.append(dict(route=r, negatives_per_positive=seen, epoch_ms=round(med * 1e3, 3),
                         epoch_ms_range=[round(min(times[r]) * 1e3, 3),
                                         round(max(times[r]) * 1e3, 3)],
                         epoch_ms_per_negative=round(med * 1e3 / seen, 5),
                         mean_loss_last_epoch=round(losses[r], 6)))
        print(json.dumps(rows[-1]), flush=True)
    if a.profile_only:
        return
    tag = _capi.load().spfm_build_tag().decode()
    out = dict(
        tool="bench_pairwise_inbatch", build_tag=tag, device=eng["in_batch"].device_name,
        contexts=B, candidates=C, features=d, k=k, positives=Q, batch=a.batch, warmup=a.warmup,
        runs=a.runs, updates_per_epoch=-(-Q // a.batch),
        context_entries_mean=round(X.nnz / B, 2), candidate_entries_mean=round(Z.nnz / C, 2),
        by_route=rows,
        routes=dict(in_batch="spfm_psgd_inbatch_epoch, batch positives per minibatch",
                    softmax_M="spfm_psgd_lists_epoch, SPFM_LIST_SOFTMAX, batch lists of M "
                              "uniform negatives over the same positives"),
        timing="host clock around an epoch call that ends in a device synchronise; every route "
               "includes the upload of its list (8 m bytes of pairs, 12 m M bytes of triples); "
               "median and min .. max of the runs, routes interleaved")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "pairwise_inbatch_%s.json" % tag), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for r in routes:
        eng[r].close()


if __name__ == "__main__":
    main()
