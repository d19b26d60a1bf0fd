"""Per-call times of averagedParticleLevelset and improvedParticleLevelset (defaults: radiusFactor 1, one smoothing round of each
kind) beside unionParticleLevelset on the same particles and index: the yardstick has the same traversal and less arithmetic.  Two
states: scenes/flip01_simple.py's loop at 128^3 (bench.py's config 3, about 3.8 M particles) and scenes/benchmark_dam.py's at
379x356x124 (bench.py's config 4, about 8.3 M particles), each a few steps into its run.  The three calls are alternated; every
timed window ends in a device synchronise; medians of --calls calls after --warmup.  Prints one JSON line and writes it to
<out>/partls_time.json; with --stats, a child process first runs the 128^3 calls alone under `rocprofv3 --kernel-trace --stats`
and its kernel table becomes <out>/partls_kernel_stats.csv (the gather kernel's share of the calls is read from it).

  python tools/partls_time.py [--warmup 5] [--calls 10] [--states flip01:dam] [--out profiles] [--stats]
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

CALLS = ("unionParticleLevelset", "averagedParticleLevelset", "improvedParticleLevelset")


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
    for _ in range(steps):
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
    return dict(s=s, flags=flags, parts=pp, keep=(pv, vel, velOld, w, pres))


def dam_state(m, steps=4):
    """bench.py's config 4 (benchmark_dam.py at res 116: 379 x 356 x 124), `steps` steps in"""
    import bench
    from mantaflow_amd import core, plugins, scene
    sc = bench.dam_scene(core, plugins, scene, bench.DAM_RES)
    for _ in range(steps):
        sc["step"]()
    return dict(s=sc["s"], flags=sc["flags"], parts=sc["parts"], keep=sc)


def time_state(m, torch, st, warmup, calls):
    import numpy as np
    s, flags, pp = st["s"], st["flags"], st["parts"]
    pindex, gpi, phi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid), s.create(m.LevelsetGrid)
    m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
    fns = {"unionParticleLevelset": lambda: m.unionParticleLevelset(pp, pindex, flags, gpi, phi),
           "averagedParticleLevelset": lambda: m.averagedParticleLevelset(pp, pindex, flags, gpi, phi),
           "improvedParticleLevelset": lambda: m.improvedParticleLevelset(pp, pindex, flags, gpi, phi)}
    ts = {k: [] for k in CALLS}
    for r in range(warmup + calls):
        for k in CALLS:           # alternated: the three see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[k]()
            torch.cuda.synchronize()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    out = {"dims": [flags.sx, flags.sy, flags.sz], "particles": pp.pySize(), "indexed": pindex.size(), "warmup_calls": warmup, "timed_calls": calls}
    for k in CALLS:
        a = np.asarray(ts[k])
        out[k + "_ms"] = {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}
    u = out["unionParticleLevelset_ms"]["median"]
    out["ratio_to_union"] = {k: round(out[k + "_ms"]["median"] / u, 3) for k in CALLS[1:]}
    return out


def kernel_stats(out_dir, warmup, calls):
    """the 128^3 calls alone in a child process under rocprofv3; returns the share of the gather kernel among the plugin's kernels"""
    tmp = tempfile.mkdtemp(prefix="partls_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--states", "flip01", "--warmup", str(warmup), "--calls", str(calls), "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        dst = os.path.join(out_dir, "partls_kernel_stats.csv")
        shutil.copyfile(found[0], dst)
        tot = {}
        for row in csv.DictReader(open(dst)):
            for k in ("k_partls_gather", "k_partls_correct", "k_partls_smooth", "k_union_levelset"):
                if k in row["Name"]:
                    tot[k] = tot.get(k, 0) + int(row["TotalDurationNs"])
        own = sum(v for k, v in tot.items() if k.startswith("k_partls"))
        return {"kernel_ns": tot, "gather_share_of_partls_kernels": round(tot.get("k_partls_gather", 0) / own, 3) if own else None}
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
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    stats = kernel_stats(args.out, args.warmup, args.calls) if args.stats else None       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("partls_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "states": {}}
    for name in args.states.split(":"):
        st = {"flip01": flip01_state, "dam": dam_state}[name](m)
        torch.cuda.synchronize()
        out["states"][name] = time_state(m, torch, st, args.warmup, args.calls)
        del st
        torch.cuda.empty_cache()
    if stats:
        out["rocprofv3_flip01"] = stats
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "partls_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
