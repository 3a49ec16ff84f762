"""Batched genetic algorithm throughput (csrc/kernels/ga_batch.hip) -> profiles/ga_batch_probe.json.

For 16384 runs at the class defaults (Npop 100, maxGenerations capped at 200 for the probe) in the
box [-2, 2]^n from x0 = -1, run s on the stream 1000 + s, of Rosenbrock n = 2, 5, 10 and the
synthetic quadratic n = 5: the "ga_batch" timer of one launch (HIP events around the kernel; after
a warm-up launch, the median and the range of the repetitions) in runs/s, the mean and the largest
generation count, the mean evaluations, the best fOpt over the batch and the stuck runs; and for
scale two baselines on the first 32 of the same runs, one at a time -- the host class with device
evaluation (GeneticAlgorithm through pnol_run_ga on the same device objective: one launch round
trip per generation) and the CPU oracle (oracle.ga_findmin, one thread, each call through ctypes)
-- each as runs/s, with a check that they give the kernel's bits.  Also what the compiler made of
the kernels (registers, scratch, static LDS).  Untuned: the first measurement of this kernel.
argv: [--nrun N] [--reps K] [--nbase N] [--out FILE]."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
from parallelnonlinearoptimizationlibrary_amd import _lib as L  # noqa: E402
from parallelnonlinearoptimizationlibrary_amd.device import (Context, DeviceObjective, _dptr, _ptr,  # noqa: E402
                                                             run_ga)

PARAMS = (100, 200, 0.1, 0.3, 0.2, 0.5, 0.01, 0.5, 50, 0)   # GeneticAlgorithm's defaults, 200 generations
LB, UB, X0, SEED = -2.0, 2.0, -1.0, 1000
CASES = {"rosenbrock_n2": (L.OBJ_ROSENBROCK, 2), "rosenbrock_n5": (L.OBJ_ROSENBROCK, 5),
         "rosenbrock_n10": (L.OBJ_ROSENBROCK, 10), "quadratic_n5": (L.OBJ_QUADRATIC, 5)}
KIND_NAMES = {0: "rosenbrock", 1: "power", 4: "quadratic"}


def timer_ms(ctx, name):
    ms, cnt = C.c_double(), C.c_int()
    L.check(L.lib().pnol_ctx_timer(ctx.h, name.encode(), C.byref(ms), C.byref(cnt)), "pnol_ctx_timer")
    return ms.value, cnt.value


def probe_case(ctx, oracle, name, kind, n, nrun, reps, nbase):
    t = ctx.torch
    dev = f"cuda:{ctx.device}"
    obj = (DeviceObjective.synthetic(ctx, kind, n) if kind == L.OBJ_QUADRATIC else DeviceObjective(ctx, kind, n))
    p = np.array(PARAMS, dtype=np.float64)
    lbh, ubh = np.full(n, LB), np.full(n, UB)
    lb, ub = ctx.tensor(lbh), ctx.tensor(ubh)
    x0 = ctx.tensor(np.full((nrun, n), X0))
    f0, fo = ctx.empty(nrun), ctx.empty(nrun)
    gens = t.empty(nrun, dtype=t.int32, device=dev)
    evals = t.empty(nrun, dtype=t.int64, device=dev)
    info = t.empty(nrun, dtype=t.int32, device=dev)
    ms = []
    for rep in range(-1, reps):   # rep -1: the warm-up
        X = x0.clone()
        ctx.synchronize()
        L.check(L.lib().pnol_ctx_reset_timers(ctx.h), "pnol_ctx_reset_timers")
        L.check(L.lib().pnol_ga_batch_solve_d(ctx.h, obj.h, _dptr(p), SEED, _ptr(lb), _ptr(ub), nrun, _ptr(X),
                                              _ptr(f0), _ptr(fo), _ptr(gens), _ptr(evals), _ptr(info)),
                "pnol_ga_batch_solve_d")
        ctx.synchronize()
        total, count = timer_ms(ctx, "ga_batch")
        assert count == 1
        if rep >= 0:
            ms.append(total)
    Xh, g, ev, foh, f0h, inf = (a.cpu().numpy() for a in (X, gens, evals, fo, f0, info))
    med = statistics.median(ms)
    chunks = -(-int(PARAMS[0]) // 64)
    res = dict(kind=KIND_NAMES[kind], n=n, box=[LB, UB], x0=X0, seed=SEED, nrun=nrun, params=list(PARAMS),
               ga_batch_timer_ms=dict(median=med, min=min(ms), max=max(ms), reps=len(ms)),
               runs_per_s=nrun / (med * 1e-3), mean_generations=float(g.mean()), max_generations=int(g.max()),
               mean_evals=float(ev.mean()), best_fopt=float(np.min(foh)), median_fopt=float(np.median(foh)),
               stuck_runs=int((inf & L.GA_BATCH_STUCK).astype(bool).sum()),
               lds_bytes_per_workgroup=chunks * 64 * (8 * (2 * n + 3) + 4))
    if nbase > 0:
        baselines(oracle, obj, kind, n, lbh, ubh, Xh, f0h, foh, g, ev, min(nbase, nrun), res)
    obj.close()
    print(name, json.dumps(res), flush=True)
    return res


def baselines(oracle, obj, kind, n, lbh, ubh, Xh, f0h, foh, g, ev, nbase, res):
    """The host class with device evaluation and the CPU oracle on the first nbase runs."""
    x0 = [X0] * n
    same = True
    t0 = time.perf_counter()
    for s in range(nbase):
        Xs, r = run_ga(obj, x0, lbh, ubh, list(PARAMS), SEED + s, which=0)
        same = same and Xs.tobytes() == Xh[s].tobytes() and r.f0 == f0h[s] and r.fopt == foh[s] and \
            (r.iters, r.evals) == (g[s], ev[s])
    dt = time.perf_counter() - t0
    res["host_class_device_eval"] = dict(runs=nbase, seconds=dt, runs_per_s=nbase / dt,
                                         bitwise_equal_to_batch=bool(same))
    oobj = oracle.quadratic(n) if kind == L.OBJ_QUADRATIC else oracle.rosenbrock(n)
    same = True
    t0 = time.perf_counter()
    for s in range(nbase):
        Xs, r, st = oracle.ga_findmin(oobj, x0, lbh, ubh, list(PARAMS), SEED + s)
        same = same and st == 0 and Xs.tobytes() == Xh[s].tobytes() and r.fopt == foh[s] and \
            (r.iters, r.evals) == (g[s], ev[s])
    dt = time.perf_counter() - t0
    res["cpu_oracle_one_thread"] = dict(runs=nbase, seconds=dt, runs_per_s=nbase / dt,
                                        bitwise_equal_to_batch=bool(same))
    res["ratio_to_host_class_device_eval"] = res["runs_per_s"] / res["host_class_device_eval"]["runs_per_s"]
    res["ratio_to_cpu_oracle_one_thread"] = res["runs_per_s"] / res["cpu_oracle_one_thread"]["runs_per_s"]


def code_object_metadata():
    """What hipcc makes of ga_batch.hip with the library's flags (-Rpass-analysis)."""
    csrc = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DPNOL_AMD_BUILDING_LIBRARY",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-c++20-extensions", "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(csrc, "kernels", "ga_batch.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        f = re.search(r"Function Name: \S*k_ga_batchILi(\d+)E", ln)
        if f:
            cur = KIND_NAMES.get(int(f.group(1)), f.group(1))
            out[cur] = {}
            continue
        v = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", ln)
        if v and cur:
            out[cur][v.group(1)] = int(v.group(2))
    if not out:
        raise RuntimeError("no kernel resource remarks from hipcc:\n" + r.stderr[-2000:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrun", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nbase", type=int, default=32, help="runs of each baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ga_batch_probe.json"))
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("ga_batch_probe: no gfx950 device visible")
    import oracle
    oracle.build()
    oracle.lib()
    ctx = Context(0)
    L.check(L.lib().pnol_ctx_enable_timers(ctx.h, 1), "pnol_ctx_enable_timers")
    res = dict(device=ctx.torch.cuda.get_device_name(0), timing='the "ga_batch" timer: HIP events around the launch',
               runs="x0 = -1 in every coordinate, run s on the stream seed + s",
               library=L.LIB_PATH.replace(ROOT, "."), status="untuned")
    for name, (kind, n) in CASES.items():
        res[name] = probe_case(ctx, oracle, name, kind, n, a.nrun, a.reps, a.nbase)
    res["code_object"] = code_object_metadata()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
