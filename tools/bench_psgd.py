#!/usr/bin/env python3
"""Timing of the psgd solver on the config-2 matrix (1M x 100k CSR,
50 nnz/row, degree 2, k = 30, batch_size 'auto' = 1/density = 2000 rows); prints one JSON
line per regularizer with the per-kernel split from the engine's HIP-event profiler.
Not the driver benchmark (bench.py).

``--learning-rate NAME`` (default ``optimal``) picks the step rule.  ``--learning-rate adagrad``
measures the per-feature AdaGrad update against the plain update ON ONE
HANDLE: after a warm-up of each, ``STEPS`` (default 5 here) epochs of the ``constant`` rule and of
the adaptive rule alternate, host clock around epoch calls that end in a device synchronise; the
medians, all repeats and the spread go to ``profiles/adagrad_<engine tag>.json`` (one entry per
regularizer; squared norms are skipped: adaptive steps refuse them).

Algorithmic HBM bytes per epoch (f32 storage of X, f64 parameters):
  gradient pass   nnz * (4 idx + 4 val) + nnz * k * (8 read P + 8 atomic add)   [P/grad rows
                  are L2/LLC-resident; counted once per touch]
  update pass     n_batches * d * k * (8+8 read, 8+8 write)   P and grad_P
  Michelot sweeps n_batches * sweeps * d * k * 8 (squaredl12) or * d * 8 (squaredl21)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsepoly_amd.engine import HipEngine  # noqa: E402
from sparsepoly_amd.synth import make_problem  # noqa: E402

n = int(os.environ.get("SPFM_BENCH_N", 1_000_000))
d = int(os.environ.get("SPFM_BENCH_D", 100_000))
k = int(os.environ.get("SPFM_BENCH_K", 30))
argv = sys.argv[1:]
rate = "optimal"
if "--learning-rate" in argv:
    at = argv.index("--learning-rate")
    rate = argv[at + 1]
    del argv[at:at + 2]
regs = argv or ["l1", "l21", "squaredl12", "squaredl21"]
X, y = make_problem(n, d, 50, 0)
Xc = X.tocsc()
Xc.sort_indices()
nnz = Xc.nnz
batch = int(os.environ.get("SPFM_BENCH_BATCH", int(n * d / nnz)))
nb = -(-n // batch)
GAMMA = {"l1": 1e-3, "l21": 1e-3, "squaredl12": 1e-6, "squaredl21": 1e-6}
cpu = None
if os.environ.get("SPFM_CPU", "0") == "1":
    # bounded CPU baseline: the oracle (single thread, f64) on the first `nbc` minibatches
    # of the same matrix with the full-width P, scaled to one epoch
    from oracle import oracle as orc

    orc.build()
    nbc = int(os.environ.get("SPFM_CPU_BATCHES", 8))
    Xs = X.tocsr()[: nbc * batch]
    Xo = orc.CSR(Xs)
    Po = np.ascontiguousarray((0.01 * np.random.RandomState(0).randn(1, k, d)).swapaxes(1, 2))
    wo = np.zeros(d)
    cpu = {}
    for reg in regs:
        t0 = time.perf_counter()
        orc.psgd_epoch(Po.copy(), wo.copy(), Xo, y[: nbc * batch], np.ones(k), 2, 1e-3, 1e-3,
                       GAMMA[reg], reg, "squared", np.arange(nbc * batch, dtype=np.int32), True,
                       0.01, "optimal", 1.0, batch, 1)
        cpu[reg] = (time.perf_counter() - t0) * nb / nbc


def compare_adagrad():
    """both update kernels on one handle, alternating; -> profiles/adagrad_<engine tag>.json"""
    from sparsepoly_amd import _capi

    steps = int(os.environ.get("STEPS", 5))
    tag = _capi.load().spfm_build_tag().decode()
    rows = []
    for reg in [r for r in regs if r in ("l1", "l21")]:
        eng = HipEngine(0, "f32")
        eng.set_data(Xc, y)
        P0 = 0.01 * np.random.RandomState(0).randn(1, k, d)
        eng.set_params(P0, np.zeros(d), np.ones(k))
        eng.configure("psgd", "squared", reg, 2)
        idx = np.arange(n, dtype=np.int32)
        args = (2, 1e-3, 1e-3, GAMMA[reg], 0.01, "constant", 1.0, batch, idx, True)
        it = 1
        times = {"constant": [], "adagrad": []}
        loss = {}
        acc = {"adagrad": (None, None)}
        for rep in range(steps + 1):  # rep 0: warm-up of both (graph capture included)
            for mode in ("constant", "adagrad"):
                # the switch (an upload and a synchronise) stays outside the timed window; the
                # adaptive epochs continue from their own accumulators
                eng.psgd_set_adaptive(int(mode == "adagrad"), 1.0, *acc.get(mode, (None, None)))
                t0 = time.perf_counter()
                sl, it = eng.psgd_epoch(*args, it)
                dt = time.perf_counter() - t0
                if mode == "adagrad":
                    acc[mode] = eng.psgd_get_adaptive()
                if rep:
                    times[mode].append(dt)
                loss[mode] = sl / n
        # one more epoch of each under the engine's HIP-event profiler (eager launches): the
        # update kernels' own times
        upd = {}
        eng.profile_enable(True)
        for mode in ("constant", "adagrad"):
            eng.psgd_set_adaptive(int(mode == "adagrad"), 1.0, *acc.get(mode, (None, None)))
            eng.profile_reset()
            sl, it = eng.psgd_epoch(*args, it)
            ms, launches, _ = eng.profile_get(1)
            upd[mode] = round(ms * 1e3 / launches, 2)
            ms, launches, _ = eng.profile_get(0)
            upd[mode + "_grad"] = round(ms * 1e3 / launches, 2)
        eng.profile_enable(False)
        med = {m: float(np.median(v)) for m, v in times.items()}
        spread = {m: float(max(v) - min(v)) for m, v in times.items()}
        row = dict(
            tool="bench_psgd --learning-rate adagrad", build_tag=tag, device=eng.device_name,
            reg=reg, n=n, d=d, k=k, batch_size=batch, updates_per_epoch=nb, warmup=1, runs=steps,
            constant_epoch_ms=round(med["constant"] * 1e3, 3),
            constant_epoch_ms_all=[round(v * 1e3, 3) for v in times["constant"]],
            adagrad_epoch_ms=round(med["adagrad"] * 1e3, 3),
            adagrad_epoch_ms_all=[round(v * 1e3, 3) for v in times["adagrad"]],
            adagrad_over_constant=round(med["adagrad"] / med["constant"], 4),
            constant_spread_ms=round(spread["constant"] * 1e3, 3),
            adagrad_spread_ms=round(spread["adagrad"] * 1e3, 3),
            update_bytes_ratio=round((4 * k + 2) / (4 * k), 4),
            profiled_us_per_batch=dict(update_constant=upd["constant"],
                                       update_adagrad=upd["adagrad"],
                                       grad_constant=upd["constant_grad"],
                                       grad_adagrad=upd["adagrad_grad"]),
            mean_loss_last_epoch={m: round(float(v), 6) for m, v in loss.items()},
            timing="host clock around an epoch call that ends in a device synchronise; the two "
                   "rules alternate on one handle, both replayed from their own hipGraph")
        rows.append(row)
        print(json.dumps(row), flush=True)
        eng.close()
    out_dir = os.environ.get("SPFM_BENCH_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "adagrad_%s.json" % tag), "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if rate == "adagrad":
    compare_adagrad()
    sys.exit(0)
for reg in regs:
    eng = HipEngine(0, "f32")
    eng.set_data(Xc, y)
    P0 = 0.01 * np.random.RandomState(0).randn(1, k, d)
    eng.set_params(P0, np.zeros(d), np.ones(k))
    eng.configure("psgd", "squared", reg, 2)
    idx = np.arange(n, dtype=np.int32)
    args = (2, 1e-3, 1e-3, GAMMA[reg], 0.01, rate, 1.0, batch, idx, True)
    sl, it = eng.psgd_epoch(*args, 1)          # warm-up epoch
    losses = [sl / n]
    steps = int(os.environ.get("STEPS", 2))
    # timed epochs: profiler off (l1 / l21 then replay runs of minibatches from a hipGraph)
    t0 = time.perf_counter()
    for _ in range(steps):
        sl, it = eng.psgd_epoch(*args, it)
        losses.append(sl / n)
    dt = (time.perf_counter() - t0) / steps
    # one more epoch under the engine's HIP-event profiler (eager launches) for the split
    split = {}
    if os.environ.get("SPFM_PROF", "1") == "1":
        eng.profile_enable(True)
        eng.profile_reset()
        sl, it = eng.psgd_epoch(*args, it)
        for which, name in ((0, "grad"), (1, "update"), (2, "prox_support")):
            ms, launches, _ = eng.profile_get(which)
            if launches:
                split[name] = dict(ms_per_epoch=round(ms, 3),
                                   us_per_batch=round(ms * 1e3 / launches, 2))
        eng.profile_enable(False)
    b_grad = nnz * 8 + nnz * k * 16
    b_upd = nb * d * k * 32
    out = dict(solver="psgd", reg=reg, k=k, batch_size=batch, batches_per_epoch=nb,
               ms_per_epoch=round(dt * 1e3, 2), epochs_per_s=round(1 / dt, 3),
               rows_per_s=round(n / dt), split=split,
               update_pass_GBs=(round(d * k * 32 / (split["update"]["us_per_batch"] * 1e-6) / 1e9, 1)
                                if "update" in split else None),
               alg_GB_per_epoch=round((b_grad + b_upd) / 1e9, 2),
               mean_loss=[round(float(v), 6) for v in losses],
               nonzero_frac_P=round(float((eng.get_params()[0] != 0).mean()), 4))
    if cpu:
        out["cpu_oracle_s_per_epoch"] = round(cpu[reg], 2)
        out["cpu_sample"] = "%d of %d minibatches, 1 thread, scaled" % (nbc, nb)
        out["gpu_over_cpu"] = round(cpu[reg] / dt, 1)
    print(json.dumps(out), flush=True)
    eng.close()
