"""Per-call times of LevelsetGrid.reinitMarching(flags, velTransport=vel) (maxTime 4) on the state of tools/tests/test_2050_freesurface.py
a few steps in, at 128^3 and 256^3.  Median, minimum and maximum of --calls calls after --warmup, each on the same restored state; every
timed window ends in a device synchronise (the call's own last read-back).  Also reported per workload: windows, sub-rounds, pops, kernel
launches and scalar read-backs of the call (inward, outward), the time of one whole free-surface step and the call's share of it, and, as
the first yardstick, the same call under MF_REINIT_SERIAL=1 (the literal loop on the host, transfers included).  Prints one JSON line and
writes it to <out>/reinit_time.json, keeping a `reference_cpu` key that tools/record_reinit.py --time put there (the second yardstick: the
compiled reference, one thread, on the CPU machine; --dump <dir> writes the 128^3 input it needs as <dir>/reinit_input_<key>.npz and
names it under `inputs`).  With --stats, a child process first runs the 128^3 calls alone under `rocprofv3 --kernel-trace --stats`; its
kernel table becomes <out>/reinit_kernel_stats.csv.

  python tools/reinit_time.py [--warmup 5] [--calls 10] [--workloads fs_128:fs_256] [--steps 3] [--out profiles] [--stats] [--dump DIR]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = {"fs_128": 128, "fs_256": 256}


def _stats(a):
    import numpy as np
    a = np.asarray(a)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


class Scene(object):
    """test_2050_freesurface.py's set-up and step"""

    def __init__(self, m, res):
        self.m, gs = m, m.vec3(res, res, res)
        s = self.s = m.Solver(name="main", gridSize=gs, dim=3)
        s.timestep = 0.25
        self.flags, self.vel, self.pressure = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid)
        self.flags.initDomain(boundaryWidth=0)
        basin = s.create(m.Box, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(1, 0.2, 1))
        drop = s.create(m.Sphere, center=gs * m.vec3(0.5, 0.5, 0.5), radius=res * 0.15)
        self.phi = basin.computeLevelset()
        self.phi.join(drop.computeLevelset())
        self.flags.updateFromLevelset(self.phi)

    def reinit(self):
        self.phi.reinitMarching(flags=self.flags, velTransport=self.vel)

    def rest(self):
        m, s, flags, vel, phi = self.m, self.s, self.flags, self.vel, self.phi
        m.advectSemiLagrange(flags=flags, vel=vel, grid=phi, order=2, clampMode=1)
        flags.updateFromLevelset(phi)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, clampMode=1)
        m.addGravity(flags=flags, vel=vel, gravity=m.vec3(0, -0.025, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=self.pressure, cgMaxIterFac=0.5, cgAccuracy=5e-5, phi=phi)
        m.setWallBcs(flags=flags, vel=vel)
        s.step()


def time_workload(m, torch, key, warmup, calls, steps, dump=None, calls_only=False):
    from mantaflow_amd import plugins
    res = WORKLOADS[key]
    sc = Scene(m, res)
    for _ in range(steps):
        sc.reinit()
        sc.rest()
    phi0, vel0 = sc.phi.data.clone(), sc.vel.data.clone()
    out = {"dims": [res] * 3, "cells": res ** 3, "steps_before": steps, "warmup_calls": warmup, "timed_calls": calls}
    if dump:
        import numpy as np
        name = "reinit_input_%s.npz" % key
        np.savez_compressed(os.path.join(dump, name), dims=np.array([res] * 3), phi=phi0.cpu().numpy(), vel=vel0.cpu().numpy(),
                            flags=sc.flags.data.cpu().numpy())
        out["input_file"] = name

    def timed(fn, n_warm, n_calls):
        ts = []
        for r in range(n_warm + n_calls):
            sc.phi.data.copy_(phi0)
            sc.vel.data.copy_(vel0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= n_warm:
                ts.append((time.perf_counter() - t0) * 1e3)
        return _stats(ts)
    out["reinitMarching_ms"] = timed(sc.reinit, warmup, calls)
    out.update(m.lastReinitStats())
    out.update(plugins._reinit_work)
    if calls_only:
        return out
    os.environ["MF_REINIT_SERIAL"] = "1"
    try:
        out["serial_path_ms"] = timed(sc.reinit, 1, 3)
        out["serial_path_pops"] = m.lastReinitStats()["pops"]
    finally:
        del os.environ["MF_REINIT_SERIAL"]

    def step():
        sc.reinit()
        sc.rest()
    out["freesurface_step_ms"] = timed(step, 1, 3)
    out["share_of_step"] = round(out["reinitMarching_ms"]["median"] / out["freesurface_step_ms"]["median"], 4)
    out["device_over_serial"] = round(out["reinitMarching_ms"]["median"] / out["serial_path_ms"]["median"], 4)
    return out


def kernel_stats(out_dir, warmup, calls, steps):
    tmp = tempfile.mkdtemp(prefix="reinit_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--workloads", "fs_128", "--warmup", str(warmup), "--calls", str(calls), "--steps", str(steps), "--no-write", "--calls-only"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        shutil.copyfile(found[0], os.path.join(out_dir, "reinit_kernel_stats.csv"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--workloads", default=":".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--dump", default=None, help="directory for the 128^3 input of the reference timing")
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the 128^3 calls (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    ap.add_argument("--calls-only", action="store_true", help="reinitMarching calls only (the traced child)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.stats:
        kernel_stats(args.out, args.warmup, args.calls, args.steps)       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("reinit_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "unit": "milliseconds", "workloads": {}, "inputs": {}}
    for key in args.workloads.split(":"):
        dump = args.dump if key == "fs_128" else None
        w = time_workload(m, torch, key, args.warmup, args.calls, args.steps, dump, args.calls_only)
        if "input_file" in w:
            out["inputs"][key] = {"file": w.pop("input_file")}
        out["workloads"][key] = w
        print(key, json.dumps(w), flush=True)
        torch.cuda.empty_cache()
    path = os.path.join(args.out, "reinit_time.json")
    if os.path.exists(path):
        old = json.load(open(path))
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    print(json.dumps(out))
    if not args.no_write:
        json.dump(out, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
