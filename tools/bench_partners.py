"""Per-feature interaction views on the device against what the package could do before them.

Config-2 parameter shape (k = 30, d = 100 000) at three active counts (d_a = 1010, 9999 and
100 000 non-zero columns), parameters only (no data set is needed):

  (a) device:   interaction_degrees, interaction_partners(K = 10) for every feature and for 4096
                features, of sparsepoly_amd.engine.HipEngine
  (b) before:   interaction_block(J, all features) in row chunks under its 1 GiB cap, then NumPy on
                the chunk: abs().sum / count_nonzero / max for the degrees, argpartition + sort of
                the K largest magnitudes for the partners.  Rows are the active features (an
                inactive row is known to be empty).  Where the rows need more than --chunks chunks
                the first --chunks are timed and the time is scaled by the row count ("scaled").

The outputs are compared first, on the rows of the first chunk: degrees and partner ids must be
equal, values equal up to the summation order (the block entry sums components one by one, the
views use the tile chain).  Every timed call ends in a synchronise (the entries return host
arrays).  Warm-up, repeats, median and spread of each; the library's build tag goes into the
output.  Writes profiles/partners_<build tag>.json unless --out is given.

    python tools/bench_partners.py [--features 100000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()),
                repeats=int(repeats))


def _chunks(rows, per):
    return [rows[i:i + per] for i in range(0, len(rows), per)]


def _before_degrees(eng, chunks, cols):
    out = []
    for J in chunks:
        M = np.abs(eng.interaction_block(0, J, cols))
        out.append((np.count_nonzero(M, axis=1), M.sum(axis=1), M.max(axis=1)))
    return out


def _before_partners(eng, chunks, cols, K):
    out = []
    for J in chunks:
        W = eng.interaction_block(0, J, cols)
        M = np.abs(W)
        part = np.argpartition(-M, K, axis=1)[:, :K]
        mag = np.take_along_axis(M, part, axis=1)
        order = np.lexsort((part, -mag), axis=1)
        ids = np.take_along_axis(part, order, axis=1)
        out.append((cols[ids], np.take_along_axis(W, ids, axis=1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--active", default="1010,9999,100000")
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--some", type=int, default=4096, help="features of the partial query")
    ap.add_argument("--chunks", type=int, default=2,
                    help="row chunks of the baseline that are timed; more are scaled")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import _capi
    from sparsepoly_amd.engine import HipEngine

    d, k, K = a.features, a.components, a.topk
    rng = np.random.RandomState(0)
    lams = np.where(rng.rand(k) < 0.5, -1.0, 1.0)
    eng = HipEngine(0, "f32")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name,
               shape=dict(features=d, components=k, topk=K, some=a.some), cases=[])
    cols = np.arange(d, dtype=np.int32)
    per = _capi.INTERACTION_BLOCK_MAX_BYTES // (8 * d)  # rows of one block under the cap
    for da in [int(v) for v in a.active.split(",")]:
        da = min(da, d)
        active = np.sort(rng.permutation(d)[:da]).astype(np.int32)
        P = np.zeros((k, d))
        P[:, active] = 0.1 * rng.randn(k, da)
        eng.set_params(P[None], np.zeros(d), lams)
        some = np.sort(rng.permutation(d)[:min(a.some, d)]).astype(np.int32)
        some_active = some[np.isin(some, active)]

        # ---- the outputs agree (rows of the first chunk)
        deg = eng.interaction_degrees(0, 0.0)
        ids, vals, counts = eng.interaction_partners(0, None, K)
        first = _chunks(active, per)[:1]
        cnt0, sum0, max0 = _before_degrees(eng, first, cols)[0]
        ids0, vals0 = _before_partners(eng, first, cols, K)[0]
        J0 = first[0]
        full = counts[J0] == K  # (the baseline's order is checked where K partners exist)
        equal = dict(
            degree=bool(np.array_equal(deg["degree"][J0], cnt0)),
            sum_abs=bool(np.allclose(deg["sum_abs"][J0], sum0, rtol=1e-11, atol=0)),
            max_abs=bool(np.allclose(deg["max_abs"][J0], max0, rtol=1e-12, atol=0)),
            partner_ids=bool(np.array_equal(ids[J0][full], ids0[full])),
            partner_vals=bool(np.allclose(vals[J0][full], vals0[full], rtol=1e-9, atol=1e-15)))
        if not all(equal.values()):
            raise SystemExit("outputs differ at d_a = %d: %s" % (da, equal))

        # ---- device
        case = dict(active_features=da, flops_per_pass=2.0 * da * da * k, outputs_equal=equal,
                    degrees=_timed(lambda: eng.interaction_degrees(0, 0.0), a.warmup, a.repeats),
                    partners_all=_timed(lambda: eng.interaction_partners(0, None, K), a.warmup,
                                        a.repeats),
                    partners_some=_timed(lambda: eng.interaction_partners(0, some, K), a.warmup,
                                         a.repeats),
                    scratch_kib=eng.get_option("interaction_scratch_kib"))

        # ---- before: dense row chunks + NumPy
        def before(rows, fn):
            ch = _chunks(rows, per)
            timed = ch[:a.chunks]
            n_timed = sum(len(c) for c in timed)
            t = _timed(lambda: fn(timed), 0, a.baseline_repeats)
            scale = len(rows) / float(n_timed)
            t.update(scaled=bool(len(ch) > len(timed)), rows=int(len(rows)),
                     rows_timed=int(n_timed), rows_per_chunk=int(per), scale=scale,
                     median_ms_full=t["median_ms"] * scale)
            return t

        case["before_degrees"] = before(active, lambda c: _before_degrees(eng, c, cols))
        case["before_partners_all"] = before(active, lambda c: _before_partners(eng, c, cols, K))
        case["before_partners_some"] = before(
            some_active, lambda c: _before_partners(eng, c, cols, K)) if len(some_active) else None
        case["ratio_before_over_device"] = dict(
            degrees=case["before_degrees"]["median_ms_full"] / case["degrees"]["median_ms"],
            partners_all=case["before_partners_all"]["median_ms_full"]
            / case["partners_all"]["median_ms"],
            partners_some=(case["before_partners_some"]["median_ms_full"]
                           / case["partners_some"]["median_ms"])
            if case["before_partners_some"] else None)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    eng.close()
    out = a.out or os.path.join(ROOT, "profiles", "partners_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
