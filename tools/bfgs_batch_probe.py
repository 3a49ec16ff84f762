"""Batched BFGS throughput (csrc/kernels/bfgs_batch.hip) -> profiles/bfgs_batch_probe.json.

For 262144 starts of Rosenbrock n = 2, 5, 10 and the synthetic quadratic n = 5, start s at
3 - 6 s / nstart in every coordinate (the standard grid's first point, spread over [-3, 3] so
that all starts are distinct), the SURVEY config-1 parameters: the wall time of one solve between
two synchronizes (after a warm-up solve; median of the repetitions) in starts/s, the mean and the
largest iteration and evaluation counts per start, and for scale two baselines on a strided
sample of the same starts -- the one-problem device path (BFGS through pnol_run_bfgs, exact
update) and the CPU oracle (oracle.bfgs_findmin, one thread, the median of 5 passes over the
sample, each call through ctypes) -- each extrapolated as starts/s, with a check that they give
the kernel's bits; and what the compiler made of the kernels
(registers, scratch, static LDS).  Untuned: the first measurement of this kernel.
argv: [--nstart N] [--reps K] [--nbase N] [--out FILE]."""
import argparse
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
                                                             run_bfgs)

PARAMS = (1e-4, 0.9, 1e-6, 1, 1000, 1e-7, 1e-3, 100, 1e-5, 1e-5, 0, 0)
CASES = {"rosenbrock_n2": (L.OBJ_ROSENBROCK, 2), "rosenbrock_n5": (L.OBJ_ROSENBROCK, 5),
         "rosenbrock_n10": (L.OBJ_ROSENBROCK, 10), "quadratic_n5": (L.OBJ_QUADRATIC, 5)}
KIND_NAMES = {0: "rosenbrock", 1: "power", 4: "quadratic"}


def starts(nstart, n):
    return np.repeat((3.0 - 6.0 * np.arange(nstart) / nstart)[:, None], n, axis=1)


def probe_case(ctx, oracle, name, kind, n, nstart, reps, nbase):
    t = ctx.torch
    dev = f"cuda:{ctx.device}"
    obj = (DeviceObjective.synthetic(ctx, kind, n) if kind == L.OBJ_QUADRATIC else DeviceObjective(ctx, kind, n))
    p = np.array(PARAMS, dtype=np.float64)
    x0h = starts(nstart, n)
    x0 = ctx.tensor(x0h)
    f0, fo, gn = ctx.empty(nstart), ctx.empty(nstart), ctx.empty(nstart)
    iters = t.empty(nstart, dtype=t.int32, device=dev)
    evals = t.empty(nstart, dtype=t.int64, device=dev)
    ms = []
    for rep in range(-1, reps):   # rep -1: the warm-up
        X = x0.clone()
        ctx.synchronize()
        t0 = time.perf_counter()
        L.check(L.lib().pnol_bfgs_batch_solve_d(ctx.h, obj.h, _dptr(p), nstart, _ptr(X), _ptr(f0), _ptr(fo), _ptr(gn),
                                                _ptr(iters), _ptr(evals)), "pnol_bfgs_batch_solve_d")
        ctx.synchronize()
        if rep >= 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    Xh, it, ev, foh, gnh = (a.cpu().numpy() for a in (X, iters, evals, fo, gn))
    med = statistics.median(ms)
    res = dict(kind=KIND_NAMES[kind], n=n, nstart=nstart, params=list(PARAMS),
               wall_ms=dict(median=med, min=min(ms), max=max(ms), reps=len(ms)), starts_per_s=nstart / (med * 1e-3),
               mean_iters=float(it.mean()), max_iters=int(it.max()), mean_evals=float(ev.mean()),
               max_evals=int(ev.max()), median_fopt=float(np.median(foh)),
               converged_fraction=float(np.mean(gnh <= PARAMS[9])), lds_bytes_per_workgroup=8 * 64 * (n * n + 6 * n))
    # baselines on a strided sample of the same starts
    idx = np.arange(0, nstart, max(nstart // nbase, 1))[:nbase]
    same = True
    t0 = time.perf_counter()
    for s in idx:
        Xs, r = run_bfgs(obj, x0h[s], list(PARAMS) + [1], which=0, profile={})   # a profile: r.iters is set
        same = same and Xs.tobytes() == Xh[s].tobytes() and r.iters == it[s] and r.evals == ev[s]
    dt = time.perf_counter() - t0
    res["one_problem_device_path"] = dict(starts=len(idx), seconds=dt, starts_per_s=len(idx) / dt,
                                          bitwise_equal_to_batch=bool(same))
    oobj = oracle.quadratic(n) if kind == L.OBJ_QUADRATIC else oracle.rosenbrock(n)
    same = True
    for s in idx:
        Xs, r, _ = oracle.bfgs_findmin(oobj, x0h[s], PARAMS)
        same = same and Xs.tobytes() == Xh[s].tobytes() and r.iters == it[s] and r.evals == ev[s]
    passes = []   # a pass is milliseconds long: the median of 5, the ctypes call included
    for _ in range(5):
        t0 = time.perf_counter()
        for s in idx:
            oracle.bfgs_findmin(oobj, x0h[s], PARAMS)
        passes.append(time.perf_counter() - t0)
    dt = statistics.median(passes)
    res["cpu_oracle_one_thread"] = dict(starts=len(idx), seconds=dt, passes=len(passes),
                                        starts_per_s=len(idx) / dt, bitwise_equal_to_batch=bool(same))
    res["ratio_to_one_problem_device_path"] = res["starts_per_s"] / res["one_problem_device_path"]["starts_per_s"]
    res["ratio_to_cpu_oracle_one_thread"] = res["starts_per_s"] / res["cpu_oracle_one_thread"]["starts_per_s"]
    obj.close()
    print(name, json.dumps(res), flush=True)
    return res


def code_object_metadata():
    """What hipcc makes of bfgs_batch.hip with the library's flags (-Rpass-analysis)."""
    csrc = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DPNOL_AMD_BUILDING_LIBRARY",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-c++20-extensions", "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(csrc, "kernels", "bfgs_batch.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        f = re.search(r"Function Name: \S*k_bfgs_batchILi(\d+)E", ln)
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
    ap.add_argument("--nstart", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nbase", type=int, default=256, help="starts of each baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfgs_batch_probe.json"))
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("bfgs_batch_probe: no gfx950 device visible")
    import oracle
    oracle.build()
    oracle.lib()
    ctx = Context(0)
    res = dict(device=ctx.torch.cuda.get_device_name(0), timing="host wall time between two synchronizes",
               starts="start s at 3 - 6 s / nstart in every coordinate", status="untuned")
    for name, (kind, n) in CASES.items():
        res[name] = probe_case(ctx, oracle, name, kind, n, a.nstart, a.reps, a.nbase)
    res["code_object"] = code_object_metadata()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
