"""Gram matrices / poly_predict of sparsepoly_amd.kernels on the config-2 matrix.

    python tools/bench_gram.py [--reps 3] [--cpu-rows 20000] [--out profiles] [--no-rocprof]

X = sparsepoly_amd.synth config 2 (1M x 100k, ~50 nnz per row), P 30 x 100k dense.  Times
``anova_kernel`` at degrees 2 and 4 and ``poly_predict`` with the anova (degree 2) and all-subsets
kernels: wall time of each call (host clock around the whole call, which ends in a device
synchronise), then -- in a separate run of this script under ``rocprofv3 --kernel-trace
--memory-copy-trace --stats`` -- the device time of the gram kernels and of the host<->device
copies of each call (upload, compute, download).  Bytes moved are counted from the shapes and
set against the 8 TB/s HBM roofline.  CPU baseline: ``oracle.anova_kernel`` (the NumPy
restatement of the reference's kernels.py) on the first --cpu-rows rows, scaled to all rows and
labelled as scaled.  Writes profiles/gram_<engine tag>.json, .txt and the two rocprofv3 stats
files.
"""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N, D, NNZ_ROW, K = 1_000_000, 100_000, 50, 30
HBM_TBS = 8.0

CALLS = [  # name, kind, degree, with lams
    ("anova_kernel_deg2", "anova", 2, False),
    ("anova_kernel_deg4", "anova", 4, False),
    ("poly_predict_anova_deg2", "anova", 2, True),
    ("poly_predict_all_subsets", "all-subsets", 0, True),
]


def problem():
    from sparsepoly_amd.synth import make_csr

    X = make_csr(N, D, nnz_per_row=NNZ_ROW, seed=0)
    rng = np.random.RandomState(0)
    P = rng.randn(K, D) * 0.1
    lams = np.sign(rng.randn(K))
    return X, P, lams


def run_call(km, X, P, lams, kind, degree, with_lams):
    if with_lams:
        return km.poly_predict(X, P, lams, kind, degree)
    return km.anova_kernel(X, P, degree)


def traffic(nnz, n, with_lams):
    csr = nnz * 12 + (n + 1) * 8
    out = n * 8 if with_lams else n * K * 8
    pt = D * K * 8
    gathered = nnz * K * 8
    return {"csr_bytes": csr, "out_bytes": out, "pt_bytes": pt, "gathered_pt_bytes": gathered,
            "compulsory_bytes": csr + out + pt,
            "roofline_ms": (csr + out + pt) / (HBM_TBS * 1e12) * 1e3}


def timed(args):
    from sparsepoly_amd import _capi
    from sparsepoly_amd import kernels as km

    t0 = time.time()
    X, P, lams = problem()
    setup = time.time() - t0
    res = {"engine_tag": _capi.build_tag(), "shape": [N, D], "nnz": int(X.nnz), "k": K,
           "data_setup_s": round(setup, 2), "calls": {}}
    for name, kind, degree, with_lams in CALLS:
        run_call(km, X, P, lams, kind, degree, with_lams)  # warm-up
        walls = []
        for _ in range(args.reps):
            t = time.perf_counter()
            run_call(km, X, P, lams, kind, degree, with_lams)
            walls.append((time.perf_counter() - t) * 1e3)
        ent = {"wall_ms": [round(w, 2) for w in walls], "wall_ms_min": round(min(walls), 2)}
        ent.update(traffic(int(X.nnz), N, with_lams))
        res["calls"][name] = ent
        print("%-26s wall %8.1f ms (min of %d)" % (name, min(walls), args.reps), flush=True)
    if args.cpu_rows > 0:
        from oracle import oracle as orc

        Xs = X[: args.cpu_rows]
        for degree in (2, 4):
            t = time.perf_counter()
            orc.anova_kernel(Xs, P, degree)
            s = time.perf_counter() - t
            res["calls"]["anova_kernel_deg%d" % degree]["cpu_numpy_s_scaled"] = round(
                s * N / args.cpu_rows, 2)
            res["calls"]["anova_kernel_deg%d" % degree]["cpu_numpy_rows_measured"] = args.cpu_rows
            print("cpu oracle.anova_kernel deg%d: %.3f s on %d rows -> %.1f s scaled to %d rows"
                  % (degree, s, args.cpu_rows, s * N / args.cpu_rows, N), flush=True)
    return res


def child(args):
    """One call of each kind, in CALLS order, for the trace (the parent splits the trace into
    calls at the host gaps between them)."""
    from sparsepoly_amd import kernels as km

    X, P, lams = problem()
    for name, kind, degree, with_lams in CALLS:
        run_call(km, X, P, lams, kind, degree, with_lams)


def _rows(path):
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return list(csv.DictReader(f))


def rocprof(args, res):
    outdir = tempfile.mkdtemp(prefix="gram_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format",
           "csv", "-d", outdir, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
           "--child"]
    rc = subprocess.call(cmd, timeout=600)
    res["rocprof_rc"] = rc
    if rc != 0:
        print("rocprofv3 exited with %d" % rc, flush=True)
        return
    # kernel_trace: one row per launch; the calls run in CALLS order
    kt = _rows(os.path.join(outdir, "run_kernel_trace.csv"))
    mt = _rows(os.path.join(outdir, "run_memory_copy_trace.csv"))
    ks = [r for r in kt if "gram_" in r.get("Kernel_Name", "")]
    ks.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the calls are separated by host work (conversion, handle creation): cut at the 3 largest gaps
    gaps = sorted(range(1, len(ks)), key=lambda i: int(ks[i]["Start_Timestamp"]) -
                  int(ks[i - 1]["End_Timestamp"]), reverse=True)[: len(CALLS) - 1]
    cuts = [0] + sorted(gaps) + [len(ks)]
    for ci, (name, _, _, _) in enumerate(CALLS):
        grp = ks[cuts[ci]: cuts[ci + 1]]
        if not grp:
            continue
        t0, t1 = int(grp[0]["Start_Timestamp"]), int(grp[-1]["End_Timestamp"])
        kern_ms = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in grp) / 1e6
        # this call's uploads: after the previous call's kernels, before this call's first
        # kernel; its downloads: after its first kernel, before the next call's first kernel
        prev_end = int(ks[cuts[ci] - 1]["End_Timestamp"]) if cuts[ci] > 0 else 0
        nxt = int(ks[cuts[ci + 1]]["Start_Timestamp"]) if cuts[ci + 1] < len(ks) else 1 << 62
        up = down = 0.0
        for r in mt:
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            direction = r.get("Direction", "")
            if "HOST_TO_DEVICE" in direction and prev_end <= s < t0:
                up += (e - s) / 1e6
            elif "DEVICE_TO_HOST" in direction and t0 <= s < nxt:
                down += (e - s) / 1e6
        ent = res["calls"][name]
        ent.update({"kernel_ms": round(kern_ms, 3), "kernel_launches": len(grp),
                    "kernel_span_ms": round((t1 - t0) / 1e6, 3),
                    "upload_ms": round(up, 2), "download_ms": round(down, 2),
                    "kernel_share_of_hbm_roofline": round(ent["roofline_ms"] / kern_ms, 3)
                    if kern_ms > 0 else None,
                    "kernel_name": grp[0]["Kernel_Name"][:90]})
    os.makedirs(args.out, exist_ok=True)
    for f in ("kernel_stats.csv", "memory_copy_stats.csv"):
        src = os.path.join(outdir, "run_" + f)
        if os.path.exists(src):
            dst = "gram_%s_%s" % (res["engine_tag"], f)
            shutil.copyfile(src, os.path.join(args.out, dst))
            res.setdefault("stats_files", []).append(dst)
    shutil.rmtree(outdir, ignore_errors=True)


def report(res):
    lines = ["sparsepoly_amd.kernels on config 2 (X %d x %d, nnz %d; P %d x %d dense), engine %s"
             % (N, D, res["nnz"], K, D, res["engine_tag"]), ""]
    hdr = "%-26s %9s %9s %9s %9s %11s %10s %10s" % (
        "call", "wall ms", "upload", "kernel", "download", "compulsory", "roofline", "cpu (s)")
    lines += [hdr, "-" * len(hdr)]
    for name, _, _, _ in CALLS:
        e = res["calls"][name]
        lines.append("%-26s %9.1f %9s %9s %9s %9.2fGB %8.3fms %10s" % (
            name, e["wall_ms_min"], e.get("upload_ms", "-"), e.get("kernel_ms", "-"),
            e.get("download_ms", "-"), e["compulsory_bytes"] / 1e9, e["roofline_ms"],
            ("%.1f*" % e["cpu_numpy_s_scaled"]) if "cpu_numpy_s_scaled" in e else "-"))
    lines += ["", "upload / kernel / download: device time of the copies and kernels of one call "
              "(rocprofv3 --kernel-trace --memory-copy-trace, separate run);",
              "roofline: compulsory bytes (CSR + output + P^T) at %.0f TB/s; the gathered P^T rows "
              "(nnz x k x 8 B) come from L2 / Infinity Cache." % HBM_TBS,
              "* oracle.anova_kernel (NumPy) on a row subset, scaled to all rows."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-rows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    res = timed(args)
    if not args.no_rocprof:
        rocprof(args, res)
    txt = report(res)
    print(txt)
    os.makedirs(args.out, exist_ok=True)
    base = os.path.join(args.out, "gram_%s" % res["engine_tag"])
    with open(base + ".json", "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    with open(base + ".txt", "w") as f:
        f.write(txt + "\n")
    print(json.dumps({"engine_tag": res["engine_tag"],
                      "calls": {k: v["wall_ms_min"] for k, v in res["calls"].items()}}))


if __name__ == "__main__":
    main()
