"""Batched Levenberg-Marquardt throughput (csrc/kernels/lm_batch.hip) -> profiles/lm_batch_probe.json.

For ExpCurve and Cubic at nprob = 262144, m = 100 on one shared grid, with each kind's example
parameters (Examples.cpp:378-450): the "lm_batch" timer of one solve for both staging shapes --
32-row chunks of y through LDS, re-read twice per trip, against all 100 rows resident in LDS
for the whole solve (PNOL_LMB_ROWS), and the library's own choice -- alternating, after a
warm-up of each, with a check that all give the same bits; the library's
one-problem device path on 32 of the same problems (host clock around whole solves) as the
baseline; and what the compiler made of the kernels (registers, scratch, static LDS).
argv: [--nprob N] [--reps K] [--out FILE]."""
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
from parallelnonlinearoptimizationlibrary_amd.device import (Context, DeviceObjective, LMBatch,  # noqa: E402
                                                             run_levmarq)

M = 100
SHAPES = {"chunk32": 32, "resident": M, "default": None}   # PNOL_LMB_ROWS (None: unset, the library's choice)
KINDS = {
    "expcurve": dict(kind=L.OBJ_EXPCURVE, n=3, params=(0.001, 10, 1e-6, 100, 1e-6, -1), coef=(10.2, 0.4, 0.1),
                     spread=0.2, noise=0.01, grid=(0.0, 5.0)),
    "cubic": dict(kind=L.OBJ_CUBIC, n=4, params=(0.001, 10, 1e-6, 10, 1e-5, -1), coef=(0.3, 1.1, -4.3, 7.3),
                  spread=0.5, noise=0.05, grid=(-5.0, 5.0)),
}


def make_data(k, nprob, rng):
    xd = np.linspace(*k["grid"], M)
    c = np.array(k["coef"])[None, :] * (1 + k["spread"] * rng.standard_normal((nprob, k["n"])))
    if k["kind"] == L.OBJ_EXPCURVE:
        y = c[:, 0:1] * np.exp(c[:, 1:2] * xd[None, :]) + c[:, 2:3]
    else:
        y = c[:, 0:1] * xd ** 3 + c[:, 1:2] * xd ** 2 + c[:, 2:3] * xd + c[:, 3:4]
    y += k["noise"] * rng.standard_normal((nprob, M))
    return xd, np.ascontiguousarray(y)


def timer_ms(ctx, name):
    ms, cnt = C.c_double(), C.c_int()
    L.check(L.lib().pnol_ctx_timer(ctx.h, name.encode(), C.byref(ms), C.byref(cnt)), "pnol_ctx_timer")
    return ms.value, cnt.value


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), reps=len(v))


def probe_kind(ctx, name, k, nprob, reps, rng):
    t = ctx.torch
    xd, y = make_data(k, nprob, rng)
    y_t = ctx.tensor(y)
    x0_t = t.full((nprob, k["n"]), 0.1, dtype=t.float64, device=y_t.device)
    b = LMBatch(ctx, k["kind"], M, nprob, xd)
    ms = {s: [] for s in SHAPES}
    outs = {}
    for rep in range(-1, reps):   # rep -1: the warm-up of each shape
        for s, rows in SHAPES.items():
            os.environ.pop("PNOL_LMB_ROWS", None)
            if rows is not None:
                os.environ["PNOL_LMB_ROWS"] = str(rows)
            X = x0_t.clone()
            ctx.synchronize()
            L.check(L.lib().pnol_ctx_reset_timers(ctx.h), "pnol_ctx_reset_timers")
            out = b.solve(y_t, X, k["params"])
            ctx.synchronize()
            if rep >= 0:
                ms[s].append(timer_ms(ctx, "lm_batch")[0])
            outs[s] = out
    os.environ.pop("PNOL_LMB_ROWS", None)
    X = {s: outs[s][0].cpu().numpy() for s in SHAPES}
    iters = outs["chunk32"][3].cpu().numpy()
    evals = outs["chunk32"][4].cpu().numpy()
    res = dict(nprob=nprob, m=M, params=list(k["params"]),
               shapes_bitwise_equal=all(X[s].tobytes() == X["chunk32"].tobytes() for s in SHAPES),
               mean_iters=float(iters.mean()), mean_residual_evals_per_problem=float(evals.mean()),
               nan_problems=int(np.isnan(X["chunk32"]).any(axis=1).sum()))
    for s in SHAPES:
        st = stats(ms[s])
        res[s] = dict(ms=st, fits_per_s=nprob / (st["median"] * 1e-3))
    # baseline: the one-problem device path on 32 of the same problems (one warm-up solve first)
    nb = 32
    objs = [DeviceObjective(ctx, k["kind"], k["n"], M, xd, y[p]) for p in range(nb)]
    run_levmarq(objs[0], np.full(k["n"], 0.1), k["params"])
    same = True
    t0 = time.perf_counter()
    Xs = [run_levmarq(o, np.full(k["n"], 0.1), k["params"])[0] for o in objs]
    dt = time.perf_counter() - t0
    for p in range(nb):
        same = same and Xs[p].tobytes() == X["chunk32"][p].tobytes()
    res["one_problem_path"] = dict(problems=nb, seconds=dt, fits_per_s=nb / dt, bitwise_equal_to_batch=same)
    for s in SHAPES:
        res[s]["ratio_to_one_problem_path"] = res[s]["fits_per_s"] / (nb / dt)
    b.close()
    print(name, json.dumps(res), flush=True)
    return res


def code_object_metadata():
    """What hipcc makes of lm_batch.hip with the library's flags (-Rpass-analysis)."""
    csrc = os.path.join(ROOT, "parallelnonlinearoptimizationlibrary_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DPNOL_AMD_BUILDING_LIBRARY",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, "-Wno-c++20-extensions", "--offload-arch=gfx950",
           "-munsafe-fp-atomics", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(csrc, "kernels", "lm_batch.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        f = re.search(r"Function Name: \S*k_lm_batchILi(\d+)ELb(\d)E", ln)
        if f:
            cur = ("expcurve" if f.group(1) == "10" else "cubic") + ("_per_problem_grid" if f.group(2) == "1" else "_shared_grid")
            out[cur] = {}
            continue
        v = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", ln)
        if v and cur:
            out[cur][v.group(1)] = int(v.group(2))
    if not out:
        raise RuntimeError("no kernel resource remarks from hipcc:\n" + r.stderr[-2000:])
    for name, d in out.items():
        narr = 1 + (0 if name.endswith("_shared_grid") else (2 if name.startswith("cubic") else 1))
        d["dynamic_LDS_bytes_chunk32"] = 8 * narr * 64 * 33
        d["dynamic_LDS_bytes_resident_m100"] = 8 * narr * 64 * 101
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_batch_probe.json"))
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("lm_batch_probe: no gfx950 device visible")
    ctx = Context(0)
    L.check(L.lib().pnol_ctx_enable_timers(ctx.h, 1), "pnol_ctx_enable_timers")
    rng = np.random.default_rng(20261020)
    res = dict(device=ctx.torch.cuda.get_device_name(0), timer="lm_batch (device events around the launch)")
    for name, k in KINDS.items():
        res[name] = probe_kind(ctx, name, k, a.nprob, a.reps, rng)
    res["code_object"] = code_object_metadata()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
