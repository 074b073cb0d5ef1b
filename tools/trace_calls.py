"""Calls into the HIP runtime of a small fit plus one call of each read-only entry: the program
for one rocprofv3 trace, and the summary of that trace.

    rocprofv3 --hip-trace --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/trace_calls.py
    python tools/trace_calls.py --summarise DIR > profiles/<name>_call_stats.json

The trace is a run of its own (no counters).  The summary holds the call counts of the runtime
entries that host plumbing can change and the launch count of every kernel, so two builds can be
compared with `diff`.
"""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RUNTIME_CALLS = ("hipStreamSynchronize", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipMalloc",
                 "hipFree", "hipMemsetAsync", "hipLaunchKernel", "hipModuleLaunchKernel",
                 "hipExtModuleLaunchKernel", "hipGraphLaunch", "hipMemcpy")


def program():
    import numpy as np
    import scipy.sparse as sp

    from sparsepoly_amd.engine import HipEngine

    rng = np.random.RandomState(11)
    n, d, k = 300, 40, 4
    X = sp.random(n, d, density=0.15, random_state=rng, format="csr")
    X.sort_indices()
    y = rng.randn(n)
    Xh = sp.random(50, d, density=0.15, random_state=rng, format="csr")
    Xh.sort_indices()
    lams = np.array([1.0, -1.0, 1.0, -1.0])
    for dtype in ("f32", "f64"):
        for solver, reg in (("pcd", "l1"), ("pbcd", "l21")):
            eng = HipEngine(0, dtype)
            eng.set_data(X, y)
            eng.set_params(rng.randn(1, k, d) * 0.1, np.zeros(d), lams)
            eng.configure(solver, "squared", reg, 2)
            eng.set_schedule("colored", rng.permutation(d).astype(np.int32))
            eng.init_pred(2, True, False)
            for _ in range(3):
                eng.cd_linear_epoch(0.1)
                if solver == "pcd":
                    eng.pcd_epoch(0, 2, 0.1, 1e-3, 1.0, np.arange(k, dtype=np.int32))
                else:
                    eng.pbcd_epoch(0, 2, 0.1, 1e-3, 1.0)
            # one call of each read-only entry
            eng.get_y_pred()
            eng.loss_sum()
            eng.get_params()
            eng.predict(Xh, 2, True, False)
            eng.objective_terms(0, 2)
            eng.objective_terms(-1, 2)
            eng.set_eval_data(Xh, rng.randn(50))
            eng.eval_loss(2, True, False, return_pred=True)
            eng.interaction_stats(0, 0.0)
            eng.interaction_topk(0, 5)
            eng.interaction_list(0, 0.0, d * d)
            eng.interaction_values(0, np.arange(5), np.arange(5) + 1)
            eng.interaction_block(0, np.arange(6))
            follower = HipEngine(0, dtype)
            follower.share_data(eng, -y)
            follower.close()
            eng.close()
    from sparsepoly_amd import kernels

    Bd = rng.randn(70, d)  # 70 columns: two 64-column chunks
    for kind, deg in (("anova", 3), ("poly", 2), ("all-subsets", 0)):
        kernels._gram(X, Bd, kind, deg)
        kernels._gram(X, Xh, kind, deg)
        kernels._gram(X, Bd, kind, deg, lams=np.ones(70), max_block_bytes=4096)
    print("trace program done")


def summarise(directory):
    def rows(pattern):
        files = sorted(glob.glob(os.path.join(directory, "**", pattern), recursive=True))
        if not files:
            raise SystemExit("no %s under %s" % (pattern, directory))
        with open(files[0]) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    api, kern = rows("*hip_api_stats.csv"), rows("*kernel_stats.csv")
    out = {"runtime_calls": {c: api.get(c, 0) for c in RUNTIME_CALLS},
           "kernel_launches_total": sum(kern.values()),
           "kernel_launches": dict(sorted(kern.items()))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        program()
