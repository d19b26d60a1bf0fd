"""Per-call times of Mesh.computeLevelset(sigma = 2) on the two reference meshes placed as the reference's scripts place them:
tools/tests/test_0050_meshload.py's mesh at its own res = 100 and scenes/meshload.py's torus at 128^3 and 256^3.  Median, minimum and
maximum of --calls calls after --warmup; every timed window ends in a device synchronise (the call's own last read-back).  Also reported
per workload: the split into source generation, binning, gather and flood fill (a second set of calls with a synchronise after each
stage, so its sum exceeds the whole call), sources generated and binned, flood rounds, the share of cells with a source in reach (cells
the gather wrote), the same call on an empty mesh as a fraction of the full call, and, as the second yardstick, averagedParticleLevelset
(k_partls_gather: a traversal of like shape) on a grid of the same size with 8 particles per cell in its lower block.  Prints one JSON
line and writes it to <out>/meshsdf_time.json, keeping a `reference_cpu` key that tools/record_meshsdf.py --time put there (the first
yardstick: the compiled reference, single-threaded as it is written, on the CPU machine).  With --stats, a child process first runs the
128^3 calls alone under `rocprofv3 --kernel-trace --stats`; its kernel table becomes <out>/meshsdf_kernel_stats.csv.

  python tools/meshsdf_time.py [--warmup 5] [--calls 10] [--workloads test0050_100:torus_128:torus_256] [--out profiles] [--stats]
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
GOLD = os.path.join(ROOT, "tests", "golden")
# name -> (.obj under tests/golden, res, the shift added to the centre)
WORKLOADS = {"test0050_100": ("test_0050_meshload.obj", 100, (0, 0, 0)), "torus_128": ("simpletorus.obj", 128, (0.1, 0.05, 0)),
             "torus_256": ("simpletorus.obj", 256, (0.1, 0.05, 0))}
STAGES = ("sources", "binning", "gather", "flood")


def _stats(a):
    import numpy as np
    a = np.asarray(a)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def setup(m, key):
    fname, res, shift = WORKLOADS[key]
    s = m.Solver(name=key, gridSize=m.vec3(res, res, res), dim=3)
    mesh, phi = s.create(m.Mesh), s.create(m.LevelsetGrid)
    mesh.load(os.path.join(GOLD, fname))
    mesh.scale(m.vec3(res / 3.0))
    mesh.offset(m.vec3(res, res, res) * (m.vec3(0.5) + m.vec3(*shift)))
    return s, mesh, phi


def time_workload(m, torch, key, warmup, calls, yardstick=True):
    from mantaflow_amd import core
    s, mesh, phi = setup(m, key)
    res = WORKLOADS[key][1]

    def timed(fn):
        ts = []
        for r in range(warmup + calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return _stats(ts)
    out = {"dims": [res] * 3, "cells": res ** 3, "triangles": mesh.numTris(), "warmup_calls": warmup, "timed_calls": calls}
    out["computeLevelset_ms"] = timed(lambda: mesh.computeLevelset(phi, 2.))
    out.update(m.lastMeshSdfStats())
    split = {k: [] for k in STAGES}
    last = [0.0]

    def mark(stage):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if stage != "start":
            split[stage].append((now - last[0]) * 1e3)
        last[0] = now
    core.Mesh._sdf_mark = mark
    try:
        for r in range(warmup + calls):
            if r == warmup:
                for k in STAGES:
                    del split[k][:]
            mesh.computeLevelset(phi, 2.)
    finally:
        core.Mesh._sdf_mark = None
    out["stage_ms_with_a_synchronise_after_each"] = {k: _stats(v) for k, v in split.items()}
    mesh._mesh_sdf(s.lib, "meshsdf_time", phi, 2., -1., flood=False)
    s.sync()
    out["share_of_cells_with_a_source_in_reach"] = float((phi.data != -4.0).float().mean().item())
    empty = s.create(m.Mesh)
    out["empty_mesh_ms"] = timed(lambda: empty.computeLevelset(phi, 2.))
    out["empty_mesh_share_of_call"] = round(out["empty_mesh_ms"]["median"] / out["computeLevelset_ms"]["median"], 4)
    if yardstick:
        flags = s.create(m.FlagGrid)
        flags.initDomain(boundaryWidth=0)
        flags.updateFromLevelset(m.Box(parent=s, p0=m.vec3(0, 0, 0), p1=m.vec3(0.4 * res, 0.6 * res, res)).computeLevelset())
        pp = s.create(m.BasicParticleSystem)
        m.sampleFlagsWithParticles(flags, pp, 2, 0.2)
        pindex, gpi, phiP = s.create(m.ParticleIndexSystem), s.create(m.IntGrid), s.create(m.LevelsetGrid)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        out["yardstick_averagedParticleLevelset_ms"] = timed(lambda: m.averagedParticleLevelset(pp, pindex, flags, gpi, phiP))
        out["yardstick_particles"] = pp.pySize()
    return out


def kernel_stats(out_dir, warmup, calls):
    tmp = tempfile.mkdtemp(prefix="meshsdf_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--workloads", "torus_128", "--warmup", str(warmup), "--calls", str(calls), "--no-write", "--calls-only"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        shutil.copyfile(found[0], os.path.join(out_dir, "meshsdf_kernel_stats.csv"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--workloads", default=":".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the 128^3 calls (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    ap.add_argument("--calls-only", action="store_true", help="computeLevelset calls only (the traced child)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.stats:
        kernel_stats(args.out, args.warmup, args.calls)       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("meshsdf_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "unit": "milliseconds", "workloads": {}}
    for key in args.workloads.split(":"):
        if args.calls_only:
            s, mesh, phi = setup(m, key)
            for _ in range(args.warmup + args.calls):
                mesh.computeLevelset(phi, 2.)
            torch.cuda.synchronize()
            out["workloads"][key] = m.lastMeshSdfStats()
        else:
            out["workloads"][key] = time_workload(m, torch, key, args.warmup, args.calls)
        torch.cuda.empty_cache()
    path = os.path.join(args.out, "meshsdf_time.json")
    if os.path.exists(path):
        old = json.load(open(path))
        if "reference_cpu" in old:
            out["reference_cpu"] = old["reference_cpu"]
    print(json.dumps(out))
    if not args.no_write:
        json.dump(out, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
