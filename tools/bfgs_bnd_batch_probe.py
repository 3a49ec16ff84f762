"""Batched box-bounded BFGS throughput (csrc/kernels/bfgs_bnd_batch.hip) ->
profiles/bfgs_bnd_batch_probe.json.

For 262144 starts of Rosenbrock n = 2, 5, 8 and the synthetic quadratic n = 5 in the box
[-1.5, 1.2]^n, on the tests' standard grid (x0[s][j] = lb + (ub - lb) mod(0.37 s + 0.21 j + 0.05, 1)),
the parameters of the reference's bounded example (Examples.cpp:75, silent): the wall time of one
solve between two synchronizes (after a warm-up solve; median of the repetitions) in starts/s, the
mean and the largest iteration and evaluation counts per start, the share of corner ends and the
recursion depths, and for scale two baselines on a strided sample of the same starts -- the
one-problem device path (BFGS_Bnd through pnol_run_bfgs, which = 2) and the CPU oracle
(oracle.bfgs_bnd_findmin_ex, one thread, the median of 5 passes over the sample, each call through
ctypes) -- each extrapolated as starts/s, with a check that they give the kernel's bits.  The
baselines take only the sampled starts that the plain-Python restatement
(tests/bfgs_bnd_reference.py) does not flag as corner ends (past one the reference's behaviour is
undefined), and the restatement's flag is checked against the kernel's info bit.  Also what the
compiler made of the kernels (registers, scratch, static LDS).  Untuned: the first measurement of
this kernel.  With PNOL_AMD_LIB set to a build made with EXTRA=-DPNOL_BFGS_BND_BATCH_NO_WAIT it is
the other arm of profiles/bfgs_bnd_batch_wait_ab.txt.
argv: [--nstart N] [--reps K] [--nbase N] [--no-baselines] [--out FILE]."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
from parallelnonlinearoptimizationlibrary_amd import _lib as L  # noqa: E402
from parallelnonlinearoptimizationlibrary_amd.device import (Context, DeviceObjective, _dptr, _ptr,  # noqa: E402
                                                             run_bfgs)

PARAMS = (1e-4, 0.8, 1e-6, 1, 1e-10, 2, 50, 1e-5, 1e-6, 1e-3, 200, 1e-5, 1e-5, 0, -1)   # Examples.cpp:75, silent
LB, UB = -1.5, 1.2
CASES = {"rosenbrock_n2": (L.OBJ_ROSENBROCK, 2), "rosenbrock_n5": (L.OBJ_ROSENBROCK, 5),
         "rosenbrock_n8": (L.OBJ_ROSENBROCK, 8), "quadratic_n5": (L.OBJ_QUADRATIC, 5)}
KIND_NAMES = {0: "rosenbrock", 1: "power", 4: "quadratic"}


def starts(nstart, n):
    s = np.arange(nstart)[:, None]
    j = np.arange(n)[None, :]
    return LB + (UB - LB) * np.mod(0.37 * s + 0.21 * j + 0.05, 1.0)


def probe_case(ctx, oracle, name, kind, n, nstart, reps, nbase):
    t = ctx.torch
    dev = f"cuda:{ctx.device}"
    obj = (DeviceObjective.synthetic(ctx, kind, n) if kind == L.OBJ_QUADRATIC else DeviceObjective(ctx, kind, n))
    p = np.array(PARAMS, dtype=np.float64)
    lbh, ubh = np.full(n, LB), np.full(n, UB)
    lb, ub = ctx.tensor(lbh), ctx.tensor(ubh)
    x0h = starts(nstart, n)
    x0 = ctx.tensor(x0h)
    f0, fo = ctx.empty(nstart), ctx.empty(nstart)
    iters = t.empty(nstart, dtype=t.int32, device=dev)
    evals = t.empty(nstart, dtype=t.int64, device=dev)
    info = t.empty(nstart, dtype=t.int32, device=dev)
    ms = []
    for rep in range(-1, reps):   # rep -1: the warm-up
        X = x0.clone()
        ctx.synchronize()
        t0 = time.perf_counter()
        L.check(L.lib().pnol_bfgs_bnd_batch_solve_d(ctx.h, obj.h, _dptr(p), _ptr(lb), _ptr(ub), nstart, _ptr(X),
                                                    _ptr(f0), _ptr(fo), _ptr(iters), _ptr(evals), _ptr(info)),
                "pnol_bfgs_bnd_batch_solve_d")
        ctx.synchronize()
        if rep >= 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    Xh, it, ev, foh, f0h, inf = (a.cpu().numpy() for a in (X, iters, evals, fo, f0, info))
    med = statistics.median(ms)
    corner = (inf & L.BFGS_BND_BATCH_CORNER) != 0
    depth = inf & 0xFF
    res = dict(kind=KIND_NAMES[kind], n=n, box=[LB, UB], nstart=nstart, params=list(PARAMS),
               wall_ms=dict(median=med, min=min(ms), max=max(ms), reps=len(ms)), starts_per_s=nstart / (med * 1e-3),
               mean_iters=float(it.mean()), max_iters=int(it.max()), mean_evals=float(ev.mean()),
               max_evals=int(ev.max()), median_fopt=float(np.median(foh)), corner_end_fraction=float(corner.mean()),
               mean_depth=float(depth.mean()), max_depth=int(depth.max()),
               lds_bytes_per_workgroup=8 * 64 * (n * n + n * (n + 1) // 2 + 8 * n))
    if nbase > 0:
        baselines(oracle, obj, kind, n, x0h, lbh, ubh, Xh, f0h, foh, it, ev, depth, corner, nbase, res)
    obj.close()
    print(name, json.dumps(res), flush=True)
    return res


def baselines(oracle, obj, kind, n, x0h, lbh, ubh, Xh, f0h, foh, it, ev, depth, corner, nbase, res):
    """The one-problem device path and the CPU oracle on the strided sample's unflagged starts."""
    import bfgs_bnd_reference as R
    nstart = len(x0h)
    idx = np.arange(0, nstart, max(nstart // nbase, 1))[:nbase]
    oobj = oracle.quadratic(n) if kind == L.OBJ_QUADRATIC else oracle.rosenbrock(n)
    fn = R.oracle_fn(oracle, oobj)
    runs = [R.find_min_bnd(fn, x0h[s], lbh, ubh, PARAMS) for s in idx]
    same = all(r.flagged == bool(corner[s]) and r.X.tobytes() == Xh[s].tobytes() and r.fopt == foh[s] and
               (r.iters, r.evals, r.depth) == (it[s], ev[s], depth[s]) for s, r in zip(idx, runs))
    res["restatement"] = dict(starts=len(idx), flagged=int(sum(r.flagged for r in runs)),
                              bitwise_equal_to_batch=bool(same))
    idx = [s for s, r in zip(idx, runs) if not r.flagged]
    if not idx:
        return
    same = True
    t0 = time.perf_counter()
    for s in idx:
        Xs, r = run_bfgs(obj, x0h[s], list(PARAMS), which=2, lb=lbh, ub=ubh)
        same = same and Xs.tobytes() == Xh[s].tobytes() and r.f0 == f0h[s] and r.fopt == foh[s] and r.iters == it[s]
    dt = time.perf_counter() - t0
    res["one_problem_device_path"] = dict(starts=len(idx), seconds=dt, starts_per_s=len(idx) / dt,
                                          bitwise_equal_to_batch=bool(same))
    same = True
    for s in idx:
        Xs, r, _, d = oracle.bfgs_bnd_findmin_ex(oobj, x0h[s], lbh, ubh, PARAMS)
        same = same and Xs.tobytes() == Xh[s].tobytes() and (r.iters, r.evals, d) == (it[s], ev[s], depth[s])
    passes = []   # the median of 5 passes, the ctypes call included
    for _ in range(5):
        t0 = time.perf_counter()
        for s in idx:
            oracle.bfgs_bnd_findmin_ex(oobj, x0h[s], lbh, ubh, PARAMS)
        passes.append(time.perf_counter() - t0)
    dt = statistics.median(passes)
    res["cpu_oracle_one_thread"] = dict(starts=len(idx), seconds=dt, passes=len(passes),
                                        starts_per_s=len(idx) / dt, bitwise_equal_to_batch=bool(same))
    res["ratio_to_one_problem_device_path"] = res["starts_per_s"] / res["one_problem_device_path"]["starts_per_s"]
    res["ratio_to_cpu_oracle_one_thread"] = res["starts_per_s"] / res["cpu_oracle_one_thread"]["starts_per_s"]


def code_object_metadata():
    """What hipcc makes of bfgs_bnd_batch.hip with the library's flags (-Rpass-analysis)."""
    csrc = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DPNOL_AMD_BUILDING_LIBRARY",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-c++20-extensions", "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(csrc, "kernels", "bfgs_bnd_batch.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        f = re.search(r"Function Name: \S*k_bfgs_bnd_batchILi(\d+)E", ln)
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
    ap.add_argument("--no-baselines", action="store_true", help="the batch timings only (an A/B arm)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfgs_bnd_batch_probe.json"))
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("bfgs_bnd_batch_probe: no gfx950 device visible")
    import oracle
    oracle.build()
    oracle.lib()
    ctx = Context(0)
    res = dict(device=ctx.torch.cuda.get_device_name(0), timing="host wall time between two synchronizes",
               starts="x0[s][j] = lb + (ub - lb) mod(0.37 s + 0.21 j + 0.05, 1)", library=L.LIB_PATH.replace(ROOT, "."),
               status="untuned")
    for name, (kind, n) in CASES.items():
        res[name] = probe_case(ctx, oracle, name, kind, n, a.nstart, a.reps, 0 if a.no_baselines else a.nbase)
    if not a.no_baselines:
        res["code_object"] = code_object_metadata()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
