"""Consensus interactions of a regularisation path: ModelBank.interaction_frequency_stats and
stable_interactions against one est.interactions(tol) call per member and a sparse merge on the
host.

F = 20 members (degree 2, k = 30) over d = 100 000 features; about 10 000 features are active in
member 0 and the supports shrink along the path (nested, down to half), as an L1-type penalty
leaves them.  tol keeps a fraction of a percent of a member's pairs, so that the lists stay below
the default max_pairs.  f64 handle, one process.  The sides alternate, warm, every call ending in
a device synchronise; per side the median, minimum and maximum wall time of --repeats rounds after
--warmup.

  (a) host:  per member est.interactions(tol) -- a handle, an upload of its parameters, a pass, its
             pair list to the host -- then count = sum_f sign(|W_f|), sum = sum_f W_f as scipy CSR
             sums: the only route without the bank entries
  (b) stats: bank.interaction_frequency_stats(tol)
  (c) list:  bank.stable_interactions(min_count, tol) (its own histogram pass, then the list)

Before any timing (c) at min_count = 1 is held to (a): same pairs, same counts, sums equal to
F 2^-53 relative to sum_f |W_f| (the host adds the members in another order), and the histogram of
(b) to the counts of (a).

--profile-pass runs one stats and one list call and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_bank_interactions.py --profile-pass`;
--kernel-us N records the device time of bi_tile_kernel<BI_HIST> read off that run and derives the
fraction of the F d_u^2 k bound at the f64 matrix rate.

    python tools/bench_bank_interactions.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

F64_MATRIX_FLOPS = 78.6e12


def _path_members(F, k, d, du):
    """nested supports: member f keeps the first du (1 - f / (2 F)) features of one permutation"""
    from bench_bank import _models

    ests = _models(F, k, d, 2)
    perm = np.random.RandomState(5).permutation(d)
    sizes = []
    for f, est in enumerate(ests):
        n_f = int(du * (1.0 - f / (2.0 * F)))
        P = np.zeros_like(est.P_)
        P[:, :, perm[:n_f]] = est.P_[:, :, perm[:n_f]]
        est.P_ = P
        sizes.append(n_f)
    return ests, sizes


def _host_side(ests, tol):
    count = total = mag = None
    for est in ests:
        W = est.interactions(tol).tocsr()
        one, absW = abs(W).sign(), abs(W)
        count = one if count is None else count + one
        total = W if total is None else total + W
        mag = absW if mag is None else mag + absW
    return count, total, mag


def main():
    from bench_bank import _stats

    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--active", type=int, default=10_000)
    ap.add_argument("--components", type=int, default=30)
    ap.add_argument("--members", type=int, default=20)
    ap.add_argument("--tol", type=float, default=0.15)
    ap.add_argument("--min-count", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-us", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from sparsepoly_amd import ModelBank, _capi
    from sparsepoly_amd.engine import HipEngine

    eng = HipEngine(0, "f64")
    res = dict(build_tag=_capi.build_tag(), device_name=eng.device_name)
    eng.close()
    F, k, d, du, tol = a.members, a.components, a.features, a.active, a.tol
    ests, sizes = _path_members(F, k, d, du)
    flops = float(sum(n * n * k for n in sizes))  # 2 k flops per pair, n^2 / 2 pairs per member
    res.update(members=F, components=k, features=d, union_active=du, member_active=sizes, tol=tol,
               min_count=a.min_count, precision="f64",
               counted=dict(flops_member_supports=flops, flops_F_du2_k=float(F) * du * du * k))
    with ModelBank(ests, precision="f64") as bank:
        if a.profile_pass:
            bank.interaction_frequency_stats(tol)
            bank.stable_interactions(a.min_count, tol)
            return
        # ---- agreement first
        count, total, mag = _host_side(ests, tol)
        for m in (count, total, mag):  # one structure, the union (Gaussian sums do not cancel)
            m.sort_indices()
        assert count.nnz == total.nnz == mag.nnz
        stats = bank.interaction_frequency_stats(tol)
        r, c, cnt, _, sums = bank.stable_interactions(1, tol)
        coo = count.tocoo()
        assert np.array_equal(r, coo.row) and np.array_equal(c, coo.col)
        assert np.array_equal(cnt, coo.data.astype(np.int32))
        want_hist = np.bincount(coo.data.astype(np.int64), minlength=F + 1)
        assert np.array_equal(stats["histogram"][1:], want_hist[1:])
        assert stats["per_member"][:3].tolist() == [e.interaction_stats(tol)["nnz"]
                                                    for e in ests[:3]]
        err = np.abs(sums - total.data)
        worst = float((err / (F * 2.0 ** -53 * mag.data)).max())
        assert worst <= 1, worst
        print("bank against %d one-model calls: pairs and counts equal (%d pairs), sums within "
              "%.3g of F 2^-53 sum|W_f|" % (F, len(r), worst), flush=True)
        res.update(agreement_pairs=int(len(r)), agreement_sum_worst_fraction_of_bound=worst,
                   histogram=stats["histogram"].tolist(), per_member=stats["per_member"].tolist(),
                   listed_at_min_count=int(stats["histogram"][a.min_count:].sum()))

        # ---- the sides alternate
        calls = [("a_one_model_calls_then_host_merge", lambda: _host_side(ests, tol)),
                 ("b_bank_frequency_stats", lambda: bank.interaction_frequency_stats(tol)),
                 ("c_bank_stable_interactions", lambda: bank.stable_interactions(a.min_count, tol))]
        times = {name: [] for name, _ in calls}
        for rep in range(a.warmup + a.repeats):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if rep >= a.warmup:
                    times[name].append(t1 - t0)
        res["wall"] = {name: _stats(ts) for name, ts in times.items()}
    med = {name: v["median_ms"] for name, v in res["wall"].items()}
    res["b_over_a_median"] = med["b_bank_frequency_stats"] / med["a_one_model_calls_then_host_merge"]
    res["c_over_a_median"] = (med["c_bank_stable_interactions"]
                              / med["a_one_model_calls_then_host_merge"])
    if a.kernel_us is not None:
        res["hist_kernel_device_us"] = a.kernel_us
        res["hist_kernel_fraction_of_F_du2_k_bound"] = (
            res["counted"]["flops_F_du2_k"] / F64_MATRIX_FLOPS / (a.kernel_us * 1e-6))
    res["not_measured"] = ["other F", "other k", "single- against double-buffered staging (only "
                           "the double-buffered form was built)"]
    out = a.out or os.path.join(ROOT, "profiles", "bank_interactions_%s.json" % res["build_tag"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
