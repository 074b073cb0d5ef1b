#!/usr/bin/env python3
"""'colored' (first fit) against 'colored_rlf' on the BASELINE config-2 matrix (config 4 shares
it), in one build of the library: classes, class widths, cold set-up time, ms per pcd iteration
(config 2: degree 2, k = 30, squaredl12) and per pbcd epoch (config 4: omegacs, k = 30).  Writes
profiles/colour_rlf_<build tag>.json.  Not the driver benchmark (bench.py).

    python tools/colour_compare.py [--n 1000000] [--d 100000] [--steps 5] [--timeout 900]

Every mode runs in a child process of its own under `--timeout` seconds; after a child that
failed or ran out of time nothing more is started.  Times are host clocks around calls that end in
a device synchronise (every epoch returns its violation sum), after one warm-up iteration that
also builds the entry streams; the two modes alternate `--rounds` times so that drift of the
shared host shows up as spread between the rounds.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("colored", "colored_rlf")
K = 30


def _engine(Xc, y, solver, reg, options):
    from sparsepoly_amd.engine import HipEngine

    d = Xc.shape[1]
    eng = HipEngine(0, "f32")
    for key, val in options.items():
        eng.set_option(key, val)
    eng.set_data(Xc, y)
    eng.set_params(0.01 * np.random.RandomState(0).randn(1, K, d), np.zeros(d), np.ones(K))
    eng.configure(solver, "squared", reg, 2)
    eng.init_pred(2, True, False)
    return eng


def _timed(fn, steps):
    fn()  # warm-up: entry streams, graphs, code objects
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def child(args):
    """one mode: colour (cold), config-2 pcd iterations, config-4 pbcd epochs in the same schedule"""
    from sparsepoly_amd.synth import make_problem

    X, y = make_problem(args.n, args.d, 50, 0)
    Xc = X.tocsc()
    Xc.sort_indices()
    d = args.d
    options = dict(kv.split("=") for kv in filter(None, args.options.split(",")))
    options = {k: int(v) for k, v in options.items()}
    eng = _engine(Xc, y, "pcd", "squaredl12", options)
    t0 = time.perf_counter()
    eng.set_schedule(args.child, np.arange(d, dtype=np.int32))
    setup_s = time.perf_counter() - t0
    sched = eng.get_schedule(args.child)
    widths = np.diff(sched.batch_ptr)
    ic = np.arange(K, dtype=np.int32)

    def pcd_iteration():
        eng.cd_linear_epoch(1.0)
        eng.pcd_epoch(0, 2, 10.0, 1e-4, 1.0, ic)

    out = dict(mode=args.child, n=args.n, d=d, nnz=int(Xc.nnz), classes=int(len(widths)),
               largest_class=int(widths.max()), mean_class=round(float(widths.mean()), 2),
               cold_setup_s=round(setup_s, 3),
               coloured_on_device=int(eng.get_option("colour_device_used")),
               wide_active=int(eng.get_option("wide_active")))
    out["pcd_ms_per_iteration"] = [round(t, 2) for t in _timed(pcd_iteration, args.steps)]
    out["pcd_persistent_fallbacks"] = int(eng.get_option("persistent_fallbacks"))
    eng.close()
    if widths.max() <= 64:  # config 4 runs the same classes (its cap is 64 columns)
        eng = _engine(Xc, y, "pbcd", "omegacs", options)
        eng.install_schedule(sched)

        def pbcd_epoch():
            eng.cd_linear_epoch(1.0)
            eng.pbcd_epoch(0, 2, 1.0, 1e-3, 1.0)

        out["pbcd_ms_per_epoch"] = [round(t, 2) for t in _timed(pbcd_epoch, args.steps)]
        out["pbcd_persistent"] = int(eng.get_option("pbprb_active"))
        eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--options", default="", help="key=value,... passed to spfm_set_option")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from sparsepoly_amd import _capi

    tag = _capi.build_tag()
    runs = []
    ok = True
    for rnd in range(args.rounds):
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--n", str(args.n),
                   "--d", str(args.d), "--steps", str(args.steps), "--options", args.options]
            try:
                p = subprocess.run(cmd, timeout=args.timeout, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                runs.append(dict(mode=mode, round=rnd, error="no result within %d s" % args.timeout))
                ok = False
                break
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                runs.append(dict(mode=mode, round=rnd, error="exit status %d" % p.returncode))
                ok = False
                break
            runs.append(dict(json.loads(lines[-1][7:]), round=rnd))
            print(json.dumps(runs[-1]), flush=True)
        if not ok:
            break
    summary = {}
    for mode in MODES:
        mine = [r for r in runs if r["mode"] == mode and "error" not in r]
        if not mine:
            continue
        pcd = [t for r in mine for t in r["pcd_ms_per_iteration"]]
        pb = [t for r in mine for t in r.get("pbcd_ms_per_epoch", [])]
        summary[mode] = dict(classes=mine[0]["classes"], largest_class=mine[0]["largest_class"],
                             mean_class=mine[0]["mean_class"],
                             cold_setup_s=[r["cold_setup_s"] for r in mine],
                             pcd_ms_per_iteration_median=round(float(np.median(pcd)), 2),
                             pcd_ms_per_iteration_min_max=[min(pcd), max(pcd)],
                             pbcd_ms_per_epoch_median=round(float(np.median(pb)), 2) if pb else None,
                             pbcd_ms_per_epoch_min_max=[min(pb), max(pb)] if pb else None)
    if len(summary) == 2:
        a, b = summary["colored"], summary["colored_rlf"]
        extra_s = float(np.median(b["cold_setup_s"]) - np.median(a["cold_setup_s"]))
        gain_ms = a["pcd_ms_per_iteration_median"] - b["pcd_ms_per_iteration_median"]
        summary["classes_saved_percent"] = round(100.0 * (1 - b["classes"] / a["classes"]), 2)
        summary["extra_setup_s"] = round(extra_s, 3)
        summary["pcd_ms_saved_per_iteration"] = round(gain_ms, 2)
        summary["break_even_pcd_iterations"] = \
            round(1e3 * extra_s / gain_ms, 1) if gain_ms > 0 else None
    doc = dict(engine_tag=tag, workload="BASELINE config 2 / 4 matrix: %d x %d, ~50 entries per row"
               % (args.n, args.d), steps_per_run=args.steps, summary=summary, runs=runs)
    out = args.out or os.path.join(ROOT, "profiles", "colour_rlf_%s.json" % tag)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s" % out)
    print(json.dumps(summary))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
