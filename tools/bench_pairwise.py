#!/usr/bin/env python3
"""Timing of one epoch of the pairwise ranking fit against the only
route the library offered before it: a pointwise psgd epoch over the 2 m materialised rows
``x_b + z_c`` with labels +1 / -1 and twice the batch size, so that both make the same number
of parameter updates.  Same build, same process, the two routes interleaved; warm-up epochs
first, then the median of ``--runs`` epochs each (host clock around calls that end in a device
synchronise).  The host time to build the stacked rows is reported separately.  Not the driver
benchmark (bench.py).

Contexts: ``synth.make_csr`` rows of about 30 stored entries; candidates: an id column and up to
two of 64 attribute columns (one to three entries).  k = 30, degree 2, l1, logistic loss.

The memory claim needs no run: 12 bytes per triple against two stored rows per triple.

``--profile-only``: warm-up and ``--runs`` epochs of both routes and nothing else, for a
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
from sparsepoly_amd import _capi  # noqa: E402
from sparsepoly_amd.engine import HipEngine  # noqa: E402
from sparsepoly_amd.synth import make_csr  # noqa: E402

N_ATTR = 64


def build_sides(B, C, d_ctx, seed):
    d = d_ctx + C + N_ATTR
    Xc = make_csr(B, d_ctx, 30, seed)
    X = sp.csr_matrix((Xc.data, Xc.indices, Xc.indptr), shape=(B, d))
    rng = np.random.RandomState(seed + 1)
    n_attr = rng.randint(0, 3, size=C)
    rows = np.concatenate([np.arange(C), np.repeat(np.arange(C), n_attr)])
    cols = np.concatenate([d_ctx + np.arange(C),
                           d_ctx + C + rng.randint(0, N_ATTR, size=int(n_attr.sum()))])
    vals = np.concatenate([np.ones(C), np.round(rng.uniform(0.25, 1, int(n_attr.sum())) * 64) / 64])
    Z = sp.csr_matrix((vals, (rows, cols)), shape=(C, d))
    Z.sum_duplicates()
    Z.sort_indices()
    return X, Z


def build_stacked_rows(X, Z, t):
    """the pointwise route's data: rows x_b + z_c+ and x_b + z_c- side by side, labels +1 / -1"""
    b2 = np.repeat(t[:, 0], 2)
    c2 = t[:, 1:].ravel()
    S = (X[b2] + Z[c2]).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    return S, np.tile([1.0, -1.0], t.shape[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--contexts", type=int, default=100_000)
    ap.add_argument("--candidates", type=int, default=20_000)
    ap.add_argument("--ctx-features", type=int, default=50_000)
    ap.add_argument("--triples", type=int, default=400_000)
    ap.add_argument("--batch", type=int, default=4096, help="triples per minibatch")
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"),
                    help="directory of pairwise_<build tag>.json")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--learning-rate", default="optimal",
                    help="step rule of both routes; 'adagrad': per-feature AdaGrad steps on the "
                         "constant rate (DESIGN.md section 19d)")
    a = ap.parse_args()

    B, C, m, k = a.contexts, a.candidates, a.triples, a.k
    X, Z = build_sides(B, C, a.ctx_features, a.seed)
    d = X.shape[1]
    rng = np.random.RandomState(a.seed + 2)
    t = np.empty((m, 3), dtype=np.int32)
    t[:, 0] = rng.randint(0, B, m)
    t[:, 1] = rng.randint(0, C, m)
    t[:, 2] = (t[:, 1] + rng.randint(1, C, m)) % C
    t0 = time.perf_counter()
    S2, y2 = build_stacked_rows(X, Z, t)
    build_s = time.perf_counter() - t0

    P0 = 0.01 * np.random.RandomState(a.seed + 3).randn(1, k, d)
    adagrad = a.learning_rate == "adagrad"
    hyper = (2, 1e-3, 1e-3, 1e-4, 0.05, "constant" if adagrad else a.learning_rate, 1.0)
    pair = HipEngine(0, "f32")
    S1 = sp.vstack([X, Z], format="csr")
    S1.sort_indices()
    pair.set_data(S1, np.zeros(B + C))
    pair.set_params(P0, np.zeros(d), np.ones(k))
    pair.configure("psgd", "logistic", "l1", 2)
    ts = (t + np.array([0, B, B])).astype(np.int32)
    point = HipEngine(0, "f32")
    point.set_data(S2, y2)
    point.set_params(P0, np.zeros(d), np.ones(k))
    point.configure("psgd", "logistic", "l1", 2)
    idx = np.arange(2 * m, dtype=np.int32)
    if adagrad:
        pair.psgd_set_adaptive(1)
        point.psgd_set_adaptive(1)

    state = {"pair": 1, "point": 1}

    def run_pair():
        t0 = time.perf_counter()
        sl, state["pair"] = pair.psgd_pairs_epoch(*hyper, a.batch, ts, True, state["pair"])
        return time.perf_counter() - t0, sl / m

    def run_point():
        t0 = time.perf_counter()
        sl, state["point"] = point.psgd_epoch(*hyper, 2 * a.batch, idx, True, state["point"])
        return time.perf_counter() - t0, sl / (2 * m)

    for _ in range(a.warmup):
        run_pair()
        run_point()
    times = {"pair": [], "point": []}
    losses = {}
    for _ in range(a.runs):  # interleaved: drift of the machine hits both routes alike
        dt, losses["pair"] = run_pair()
        times["pair"].append(dt)
        dt, losses["point"] = run_point()
        times["point"].append(dt)
    assert state["pair"] == state["point"]      # the same number of parameter updates
    if a.profile_only:
        return
    tag = _capi.load().spfm_build_tag().decode()
    med = {r: float(np.median(v)) for r, v in times.items()}
    out = dict(
        tool="bench_pairwise", build_tag=tag, device=pair.device_name,
        learning_rate=a.learning_rate,
        contexts=B, candidates=C, features=d, k=k, triples=m, batch_size=a.batch,
        updates_per_epoch=-(-m // a.batch), warmup=a.warmup, runs=a.runs,
        context_entries_mean=round(X.nnz / B, 2), candidate_entries_mean=round(Z.nnz / C, 2),
        pair_epoch_ms=round(med["pair"] * 1e3, 3),
        pair_epoch_ms_all=[round(v * 1e3, 3) for v in times["pair"]],
        stacked_epoch_ms=round(med["point"] * 1e3, 3),
        stacked_epoch_ms_all=[round(v * 1e3, 3) for v in times["point"]],
        stacked_over_pair=round(med["point"] / med["pair"], 3),
        stacked_rows_build_s=round(build_s, 3),
        triples_per_s=round(m / med["pair"]),
        bytes_per_triple=dict(pair=12, stacked=round(S2.nnz * 8 / m + 2 * 8, 1)),
        mean_loss_last_epoch=dict(pair=round(losses["pair"], 6), stacked=round(losses["point"], 6)),
        timing="host clock around an epoch call that ends in a device synchronise; both routes "
               "include the upload of their visiting order (12 m / 8 m bytes)")
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "pairwise_%s%s.json" % ("adagrad_" if adagrad else "", tag))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    pair.close()
    point.close()


if __name__ == "__main__":
    main()
