"""Records what the pair and triple interaction entries return, as digests, so that a later
build can be held to the same bits (tests/test_hip_interactions_bits.py replays the file).

Every case is one seeded block (numpy.random.RandomState, the seed is in the file): interleaved
dead columns, holes inside the live ones, lams of both signs, values rounded through float32 for
f32 handles.  On one handle per (case, handle kind, launch budget) the case's calls run in order;
a call gives one record:

    call, args        which entry, with which tolerance / K
    nnz, active_features, sum_sq, sum_abs, max_abs     (stats calls; the floats as float.hex())
    n_out             entries returned (topk / list calls)
    sha256            over the little-endian bytes of the returned id arrays, then of vals
    scratch_kib       option "interaction_scratch_kib" after the call
    launches          option "interaction_launches" after the call, by budget

"tol" is a quarter of the max_abs that stats(0) returned.  The launch budget must not change
anything but the launch count: the tool refuses to write a file otherwise, and keeps one record
per call with the launch counts of all budgets.

    python tools/record_interactions.py --out FILE [--root TREE] [--only SUBSTRING]

--root: the tree whose sparsepoly_amd package (with its built library) is recorded; this one by
default.  Needs a GPU.  The wall time of every call and case is printed, not stored.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

SEED = 20261
PAIR_CALLS = (("stats", 0), ("stats", "tol"), ("topk", 10), ("topk", 1000), ("list", 0),
              ("list", "tol"))
TRIPLE_CALLS = (("stats", 0), ("stats", "tol"), ("topk", 10), ("topk", 1000), ("list", "tol"))
STATS_ONLY = (("stats", 0),)
# name, order, (d_a, d, k), handle kinds (storage, live image), budgets (0 = default), calls
CASES = (
    # diagonal and off-diagonal tile, padding
    ("pairs_70", 2, (70, 70, 5), (("f32", "P"),), (0, 1, 16), PAIR_CALLS),
    # two component chunks, holes in the ids
    ("pairs_200", 2, (200, 260, 37), (("f32", "P"), ("f64", "Pt")), (0, 1, 16), PAIR_CALLS),
    # 244 650 pairs > 65 536: the select goes past level 0
    ("pairs_700", 2, (700, 700, 5), (("f32", "P"),), (0,),
     (("stats", 0), ("stats", "tol"), ("topk", 100), ("list", "tol"))),
    # 4 371 tiles > 4 096: two reduction levels
    ("pairs_5900", 2, (5900, 5900, 1), (("f32", "P"),), (0,), STATS_ONLY),
    # all three members in one tile
    ("triples_40", 3, (40, 40, 1), (("f32", "P"),), (0,), TRIPLE_CALLS),
    # pivot inside tile tj, ta < tj
    ("triples_70", 3, (70, 70, 5), (("f32", "P"),), (0, 1, 7), TRIPLE_CALLS),
    # restaging (k > 32), 1.3 M triples: select past level 0, key lookup through ids[]; then the
    # pair calls on the same handle (the scratch is shared)
    ("triples_200", 3, (200, 260, 37), (("f32", "P"), ("f64", "Pt")), (0,),
     TRIPLE_CALLS + (("list", 0),) + tuple(("pair_" + c, a) for c, a in PAIR_CALLS)),
    # 4 495 units > 4 096: two reduction levels
    ("triples_1800", 3, (1800, 1800, 1), (("f32", "P"),), (0,), STATS_ONLY),
    # 280 840 units > 2^18: two record windows
    ("triples_7500", 3, (7500, 7500, 1), (("f32", "P"),), (0,), STATS_ONLY),
)


def case_seed(name):
    return SEED + [c[0] for c in CASES].index(name)


def make_block(name, shape, storage):
    """(P (k, d), lams): d_a of the d columns non-zero, spread over [0, d)"""
    d_a, d, k = shape
    rng = np.random.RandomState(case_seed(name))
    P = rng.randn(k, d) + 0.1 * np.sign(rng.randn(k, d))
    P *= rng.rand(k, d) < 0.8  # holes
    dead = rng.permutation(d)[:d - d_a]
    P[:, dead] = 0.0
    alive = np.setdiff1d(np.arange(d), dead)
    P[0, alive] = np.where(P[0, alive] == 0, 0.2 + rng.rand(len(alive)), P[0, alive])
    if storage == "f32":
        P = P.astype(np.float32).astype(np.float64)
    lams = np.where(np.arange(k) % 2 == 0, -1.0, 1.0)
    return P, lams


def make_handle(P, lams, storage, image, budget):
    """A handle whose live image of the block is (k, d) ("P": after set_params) or (d, k) ("Pt":
    after one pbcd epoch with step size 0 and no penalty on a one-entry matrix)."""
    from sparsepoly_amd.engine import HipEngine

    d = P.shape[1]
    eng = HipEngine(0, storage)
    eng.set_option("interaction_tile_budget", budget)
    if image == "Pt":
        X = sp.csr_matrix((np.ones(1), (np.zeros(1, dtype=int), np.zeros(1, dtype=int))),
                          shape=(1, d))
        eng.set_data(X, np.zeros(1))
    eng.set_params(P[None], np.zeros(d), lams)
    if image == "Pt":
        eng.configure("pbcd", "squared", "l21", 2)
        eng.init_pred(2, False, False)
        eng.set_schedule("exact", np.arange(d, dtype=np.int32))
        eng.pbcd_epoch(0, 2, 1.0, 0.0, 0.0)
    return eng


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays[:-1]:
        h.update(np.ascontiguousarray(a, dtype="<i4").tobytes())
    h.update(np.ascontiguousarray(arrays[-1], dtype="<f8").tobytes())
    return h.hexdigest()


def run_calls(eng, order, calls):
    """The records of `calls` on `eng`, without the launch counts' budget key."""
    records, nnz = [], {}
    tol_of = {}
    for call, arg in calls:
        pair = order == 2 or call.startswith("pair_")
        kind = call[len("pair_"):] if call.startswith("pair_") else call
        fn = getattr(eng, ("interaction_" if pair else "interaction3_") + kind)
        val = tol_of[pair] if arg == "tol" else arg
        rec = dict(call=call, args=arg)
        t0 = time.perf_counter()
        if kind == "stats":
            st = fn(0, float(val))
            if arg == 0:
                tol_of[pair] = 0.25 * st["max_abs"]
            nnz[(pair, arg)] = st["nnz"]
            rec.update(nnz=st["nnz"], active_features=st["active_features"],
                       **{key: float(st[key]).hex() for key in ("sum_sq", "sum_abs", "max_abs")})
        else:
            out = fn(0, int(val)) if kind == "topk" else fn(0, float(val), nnz[(pair, arg)])
            rec.update(n_out=int(len(out[-1])), sha256=_digest(out))
        print("  %s(%s): %.1f ms" % (call, arg, (time.perf_counter() - t0) * 1e3), flush=True)
        rec.update(scratch_kib=int(eng.get_option("interaction_scratch_kib")),
                   launches=int(eng.get_option("interaction_launches")))
        records.append(rec)
    return records


def run_case(case, kind, budget):
    name, order, shape, _, _, calls = case
    P, lams = make_block(name, shape, kind[0])
    eng = make_handle(P, lams, kind[0], kind[1], budget)
    try:
        return run_calls(eng, order, calls)
    finally:
        eng.close()


def handle_key(kind):
    return "%s_%s" % kind


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from sparsepoly_amd import _capi

    res = dict(build_tag=_capi.build_tag(), seed=SEED, cases={})
    for case in CASES:
        name, _, shape, kinds, budgets, _ = case
        if a.only not in name:
            continue
        res["cases"][name] = dict(seed=case_seed(name), shape=list(shape), handles={})
        for kind in kinds:
            merged = None
            for budget in budgets:
                t0 = time.perf_counter()
                recs = run_case(case, kind, budget)
                print("%s %s budget %d: %.1f ms" % (name, handle_key(kind), budget,
                                                    (time.perf_counter() - t0) * 1e3), flush=True)
                for r in recs:
                    r["launches"] = {str(budget): r["launches"]}
                if merged is None:
                    merged = recs
                    continue
                for m, r in zip(merged, recs):
                    m["launches"].update(r["launches"])
                    if {**r, "launches": None} != {**m, "launches": None}:
                        raise SystemExit("%s: budget %d changed a result: %r vs %r"
                                         % (name, budget, r, m))
            res["cases"][name]["handles"][handle_key(kind)] = merged
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote %s (build %s)" % (a.out, res["build_tag"]))


if __name__ == "__main__":
    main()
