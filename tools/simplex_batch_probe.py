"""Batched Nelder-Mead throughput (csrc/kernels/simplex_batch.hip) -> profiles/simplex_batch_probe.json.

For 262144 starts of Rosenbrock n = 2, 4, 10 and Power (power 2) n = 5, every start at x0 = 3 in
every coordinate, SimplexSearch's default parameters, one seed (start s draws from seed + s): the
"simplex_batch" timer of one solve (after a warm-up solve) in starts/s, the mean and the largest
iteration count per start, and, for scale, the first 256 of the same starts run one by one
through pnol_host_run_simplex on the CPU (a C callback objective evaluated in Python, so the
time is mostly the callbacks': a scale, not a tuned baseline) with a check that they give the
kernel's bits; and what the compiler made of the kernels (registers, scratch, static LDS).
argv: [--nstart N] [--reps K] [--out FILE]."""
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
sys.path.insert(0, ROOT)
from parallelnonlinearoptimizationlibrary_amd import _lib as L  # noqa: E402
from parallelnonlinearoptimizationlibrary_amd.device import (SIMPLEX_DEFAULTS, Context, DeviceObjective,  # noqa: E402
                                                             _dptr, _ptr, host_run_simplex)

SEED = 20261021
CASES = {"rosenbrock_n2": (L.OBJ_ROSENBROCK, 2), "rosenbrock_n4": (L.OBJ_ROSENBROCK, 4),
         "rosenbrock_n10": (L.OBJ_ROSENBROCK, 10), "power2_n5": (L.OBJ_POWER, 5)}
KIND_NAMES = {0: "rosenbrock", 1: "power", 4: "quadratic"}
NHOST = 256


def rosenbrock(x):
    f = 0.0
    for k in range(len(x) - 1):
        t = x[k + 1] - x[k] * x[k]
        u = 1.0 - x[k]
        f = f + (100.0 * (t * t) + u * u)
    return f


def power2(x):
    f = 0.0
    for v in x:
        f = f + v * v
    return f


def timer_ms(ctx, name):
    ms, cnt = C.c_double(), C.c_int()
    L.check(L.lib().pnol_ctx_timer(ctx.h, name.encode(), C.byref(ms), C.byref(cnt)), "pnol_ctx_timer")
    return ms.value, cnt.value


def probe_case(ctx, name, kind, n, nstart, reps):
    t = ctx.torch
    dev = f"cuda:{ctx.device}"
    obj = DeviceObjective(ctx, kind, n)
    p = np.array(SIMPLEX_DEFAULTS, dtype=np.float64)
    x0 = t.full((nstart, n), 3.0, dtype=t.float64, device=dev)
    f0, fo = ctx.empty(nstart), ctx.empty(nstart)
    iters = t.empty(nstart, dtype=t.int32, device=dev)
    evals = t.empty(nstart, dtype=t.int64, device=dev)
    ms = []
    for rep in range(-1, reps):   # rep -1: the warm-up
        X = x0.clone()
        ctx.synchronize()
        L.check(L.lib().pnol_ctx_reset_timers(ctx.h), "pnol_ctx_reset_timers")
        L.check(L.lib().pnol_simplex_batch_solve_d(ctx.h, obj.h, _dptr(p), SEED, nstart, _ptr(X), _ptr(f0), _ptr(fo),
                                                   _ptr(iters), _ptr(evals)), "pnol_simplex_batch_solve_d")
        ctx.synchronize()
        if rep >= 0:
            ms.append(timer_ms(ctx, "simplex_batch")[0])
    Xh, it, ev, foh = X.cpu().numpy(), iters.cpu().numpy(), evals.cpu().numpy(), fo.cpu().numpy()
    med = statistics.median(ms)
    res = dict(kind=KIND_NAMES[kind], n=n, nstart=nstart, params=list(SIMPLEX_DEFAULTS), seed=SEED,
               ms=dict(median=med, min=min(ms), max=max(ms), reps=len(ms)), starts_per_s=nstart / (med * 1e-3),
               mean_iters=float(it.mean()), max_iters=int(it.max()), mean_evals=float(ev.mean()),
               median_fopt=float(np.median(foh)), lds_bytes_per_workgroup=8 * 64 * ((n + 1) ** 2 + 3 * n))
    # scale: the first NHOST starts one by one on the CPU
    fn = rosenbrock if kind == L.OBJ_ROSENBROCK else power2
    nh = min(NHOST, nstart)
    same = True
    t0 = time.perf_counter()
    for s in range(nh):
        Xs, r = host_run_simplex(fn, np.full(n, 3.0), SIMPLEX_DEFAULTS, SEED + s)
        same = same and Xs.tobytes() == Xh[s].tobytes() and r.iters == it[s] and r.evals == ev[s]
    dt = time.perf_counter() - t0
    res["host_one_by_one"] = dict(starts=nh, seconds=dt, starts_per_s=nh / dt, bitwise_equal_to_batch=bool(same),
                                  objective="Python callback")
    res["ratio_to_host_one_by_one"] = res["starts_per_s"] / (nh / dt)
    obj.close()
    print(name, json.dumps(res), flush=True)
    return res


def code_object_metadata():
    """What hipcc makes of simplex_batch.hip with the library's flags (-Rpass-analysis)."""
    csrc = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DPNOL_AMD_BUILDING_LIBRARY",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-c++20-extensions", "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(csrc, "kernels", "simplex_batch.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        f = re.search(r"Function Name: \S*k_simplex_batchILi(\d+)E", ln)
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplex_batch_probe.json"))
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("simplex_batch_probe: no gfx950 device visible")
    ctx = Context(0)
    L.check(L.lib().pnol_ctx_enable_timers(ctx.h, 1), "pnol_ctx_enable_timers")
    res = dict(device=ctx.torch.cuda.get_device_name(0), timer="simplex_batch (device events around the launch)")
    for name, (kind, n) in CASES.items():
        res[name] = probe_case(ctx, name, kind, n, a.nstart, a.reps)
    res["code_object"] = code_object_metadata()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
