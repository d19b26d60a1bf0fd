"""Per-call times of LevelsetGrid.createMesh on two liquid states, with phi from unionParticleLevelset: scenes/flip01_simple.py's loop
at 128^3 (bench.py's config 3) and scenes/benchmark_dam.py's at 379x356x124 (bench.py's config 4), each a few steps into its run.
Median, minimum and maximum of --calls calls after --warmup; every timed window ends in a device synchronise.  Also reported: nodes and
triangles, the cost of the call's one 16-byte read-back (timed alone: a copy to the host plus the synchronise) and its share of the call,
and createMesh's share of one whole step of the state's loop with createMesh added to it.  Prints one JSON line and writes it to
<out>/mesh_time.json.  With --stats, a child process first runs the 128^3 calls alone under `rocprofv3 --kernel-trace --stats`; its
kernel table becomes <out>/mesh_kernel_stats.csv, and the classify pass is held against its own bytes -- 4 B read and 1 B written per
cell -- at the 8 TB/s HBM peak.  At 128^3 phi is 8 MiB and stays in the caches from call to call: that fraction is a warm-cache figure.

  python tools/mesh_time.py [--warmup 5] [--calls 10] [--states flip01:dam] [--out profiles] [--stats]
"""
import argparse
import csv
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def flip01_state(m, n=128, steps=3):
    """bench.py's config 3 (flip01_simple.py's loop, 8 particles per cell in the lower 0.4 x 0.6 x 1.0 block), `steps` steps in"""
    import numpy as np
    s = m.Solver(name="flip01", gridSize=m.vec3(n, n, n), dim=3)
    s.timestep = 0.5
    flags = s.create(m.FlagGrid)
    flags.initDomain(boundaryWidth=0)
    flags.updateFromLevelset(m.Box(parent=s, p0=m.vec3(0, 0, 0), p1=m.vec3(0.4 * n, 0.6 * n, n)).computeLevelset())
    pp = s.create(m.BasicParticleSystem)
    m.sampleFlagsWithParticles(flags, pp, 2, 0.2)
    pv = pp.create(m.PdataVec3)
    pv.from_numpy(np.random.default_rng(9832).normal(0, 0.5, (pp.pySize(), 3)).astype(np.float32))
    vel, velOld, w, pres = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.RealGrid)

    def step():
        pp.advectInGrid(flags, vel, 2, deleteInObstacle=False)
        m.mapPartsToMAC(flags, vel, velOld, pp, pv, w)
        m.extrapolateMACFromWeight(vel, w, distance=2)
        m.markFluidCells(pp, flags)
        m.addGravity(flags, vel, m.vec3(0, -0.002, 0))
        m.setWallBcs(flags, vel)
        m.solvePressure(vel, pres, flags)
        m.extrapolateMACSimple(flags, vel)
        m.flipVelocityUpdate(flags, vel, velOld, pp, pv, 0.97)
        s.step()
    for _ in range(steps):
        step()
    return dict(s=s, flags=flags, parts=pp, step=step)


def dam_state(m, steps=4):
    """bench.py's config 4 (benchmark_dam.py at res 116: 379 x 356 x 124), `steps` steps in"""
    import bench
    from mantaflow_amd import core, plugins, scene
    sc = bench.dam_scene(core, plugins, scene, bench.DAM_RES)
    for _ in range(steps):
        sc["step"]()
    return dict(s=sc["s"], flags=sc["flags"], parts=sc["parts"], step=sc["step"], keep=sc)


def _stats(a):
    import numpy as np
    a = np.asarray(a)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def time_state(m, torch, st, warmup, calls):
    s, flags, pp = st["s"], st["flags"], st["parts"]
    pindex, gpi, phi, mesh = s.create(m.ParticleIndexSystem), s.create(m.IntGrid), s.create(m.LevelsetGrid), s.create(m.Mesh)
    m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
    m.unionParticleLevelset(pp, pindex, flags, gpi, phi)

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
    out = {"dims": [flags.sx, flags.sy, flags.sz], "cells": flags.sx * flags.sy * flags.sz, "particles": pp.pySize(), "warmup_calls": warmup,
           "timed_calls": calls}
    out["createMesh_ms"] = timed(lambda: phi.createMesh(mesh))
    out["nodes"], out["triangles"] = mesh.numNodes(), mesh.numTris()
    two = torch.zeros(2, dtype=torch.int64, device=s.device)
    out["readback_alone_ms"] = timed(lambda: two.cpu())
    out["readback_share_of_createMesh"] = round(out["readback_alone_ms"]["median"] / out["createMesh_ms"]["median"], 4)

    def step_with_mesh():
        st["step"]()
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phi)
        phi.createMesh(mesh)
    out["step_with_createMesh_ms"] = timed(step_with_mesh)
    out["createMesh_share_of_step"] = round(out["createMesh_ms"]["median"] / out["step_with_createMesh_ms"]["median"], 4)
    return out


def kernel_stats(out_dir, warmup, calls):
    """the 128^3 calls alone in a child process under rocprofv3 -> per-kernel totals and the classify pass against its own bytes"""
    tmp = tempfile.mkdtemp(prefix="mesh_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--states", "flip01", "--warmup", str(warmup), "--calls", str(calls), "--no-write", "--mesh-only"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        dst = os.path.join(out_dir, "mesh_kernel_stats.csv")
        shutil.copyfile(found[0], dst)
        avg = {}
        for row in csv.DictReader(open(dst)):
            for k in ("k_classify", "k_count", "k_totals", "k_emit", "DeviceScan"):
                if k in row["Name"]:
                    avg[k] = avg.get(k, 0.0) + float(row["TotalDurationNs"]) / (warmup + calls)
        n = 128 ** 3
        res = {"kernel_ns_per_call": {k: round(v, 1) for k, v in avg.items()}, "classify_bytes": 5 * n}
        if avg.get("k_classify"):
            bw = 5 * n / (avg["k_classify"] * 1e-9)
            res["classify_TBs"] = round(bw / 1e12, 3)
            res["classify_share_of_hbm_peak_warm_cache"] = round(bw / HBM_PEAK, 3)
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--states", default="flip01:dam")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the 128^3 calls (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    ap.add_argument("--mesh-only", action="store_true", help="createMesh calls only: no read-back and whole-step windows (the traced child)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    stats = kernel_stats(args.out, args.warmup, args.calls) if args.stats else None       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_TBs": HBM_PEAK / 1e12, "states": {}}
    for name in args.states.split(":"):
        st = {"flip01": flip01_state, "dam": dam_state}[name](m)
        torch.cuda.synchronize()
        if args.mesh_only:
            s = st["s"]
            pindex, gpi, phi, mesh = s.create(m.ParticleIndexSystem), s.create(m.IntGrid), s.create(m.LevelsetGrid), s.create(m.Mesh)
            m.gridParticleIndex(parts=st["parts"], flags=st["flags"], indexSys=pindex, index=gpi)
            m.unionParticleLevelset(st["parts"], pindex, st["flags"], gpi, phi)
            for _ in range(args.warmup + args.calls):
                phi.createMesh(mesh)
            torch.cuda.synchronize()
            out["states"][name] = {"nodes": mesh.numNodes(), "triangles": mesh.numTris()}
        else:
            out["states"][name] = time_state(m, torch, st, args.warmup, args.calls)
        del st
        torch.cuda.empty_cache()
    if stats:
        out["rocprofv3_flip01"] = stats
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "mesh_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
