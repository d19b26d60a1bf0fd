"""Per-call times of the four secondary-particle plugins on two states: scenes/flip01_simple.py's loop at 128^3 (bench.py's config 3)
and scenes/benchmark_dam.py's at 379x356x124 (bench.py's config 4) after the column has broken.  Per state: the potentials at
radius 1 and 2, their two passes separately (the streaming pass against its own bytes at the HBM peak, the gather against
k_partls_gather -- averagedParticleLevelset without smoothing -- on the same grid, a traversal of like shape), "single" sampling,
the "linear" update with antitunneling 4 and flipDeleteParticlesInObstacle, the spawned and live secondary particles, and the four
calls' share of the whole step: windows of the state's step with and without them are alternated.  Every timed window ends in a
device synchronise; medians of --calls calls after --warmup.  Prints one JSON line and writes it to <out>/secparts_time.json; with
--stats, a child process first runs the 128^3 calls alone under `rocprofv3 --kernel-trace --stats` and its kernel table becomes
<out>/secparts_kernel_stats.csv.

  python tools/secparts_time.py [--warmup 5] [--calls 10] [--states flip01:dam] [--out profiles] [--stats]
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

HBM_PEAK_TBS = 8.0            # MI355X HBM3E peak, the figure the README's other sections use
PRE_BYTES_PER_CELL = 4 + 12 + 4 + 16 + 12 + 12 + 12 + 4      # flags, vel, phi in; 4 outputs, normal, two Vec3 scratch grids, class out
PAR = dict(taus=(2.0, 12.0, 1.0, 8.0, 0.02, 0.4), lMin=1.0, lMax=4.0, c_s=0.4, c_b=0.8, k_ta=40.0, k_wc=40.0, k_b=0.5, k_d=0.4,
           gravity=(0.0, -0.004, 0.0))


def flip01_state(m, n=128, steps=6):
    """bench.py's config 3 (flip01_simple.py's loop, 8 particles per cell in the lower 0.4 x 0.6 x 1.0 block), `steps` steps in"""
    s = m.Solver(name="flip01", gridSize=m.vec3(n, n, n), dim=3)
    s.timestep = 0.5
    flags = s.create(m.FlagGrid)
    flags.initDomain(boundaryWidth=0)
    flags.updateFromLevelset(m.Box(parent=s, p0=m.vec3(0, 0, 0), p1=m.vec3(0.4 * n, 0.6 * n, n)).computeLevelset())
    pp = s.create(m.BasicParticleSystem)
    m.sampleFlagsWithParticles(flags, pp, 2, 0.2)
    pv = pp.create(m.PdataVec3)
    vel, velOld, w, pres = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.RealGrid)

    def step():
        pp.advectInGrid(flags, vel, 2, deleteInObstacle=False)
        m.mapPartsToMAC(flags, vel, velOld, pp, pv, w)
        m.extrapolateMACFromWeight(vel, w, distance=2)
        m.markFluidCells(pp, flags)
        m.addGravity(flags, vel, m.vec3(0, -0.002, 0))
        m.setWallBcs(flags, vel)
        m.solvePressure(vel, pres, flags)
        m.setWallBcs(flags, vel)
        m.extrapolateMACSimple(flags, vel)
        m.flipVelocityUpdate(flags, vel, velOld, pp, pv, 0.97)
        s.step()

    for _ in range(steps):
        step()
    return dict(s=s, flags=flags, vel=vel, parts=pp, step=step, keep=(pv, velOld, w, pres))


def dam_state(m, steps=12):
    """bench.py's config 4 (benchmark_dam.py at res 116: 379 x 356 x 124), `steps` steps in"""
    import bench
    from mantaflow_amd import core, plugins, scene
    sc = bench.dam_scene(core, plugins, scene, bench.DAM_RES)
    for _ in range(steps):
        sc["step"]()
    return dict(s=sc["s"], flags=sc["flags"], vel=sc["vel"], parts=sc["parts"], step=sc["step"], keep=sc)


def time_state(m, torch, st, warmup, calls):
    import numpy as np
    from mantaflow_amd.plugins import _scratch_grid
    s, flags, vel, pp = st["s"], st["flags"], st["vel"], st["parts"]
    pindex, gpi, phi, phi2 = s.create(m.ParticleIndexSystem), s.create(m.IntGrid), s.create(m.LevelsetGrid), s.create(m.LevelsetGrid)
    normal = s.create(m.VecGrid)
    pots = [s.create(m.RealGrid) for _ in range(4)]
    sec = s.create(m.BasicParticleSystem)
    vSec, lSec, fSec = sec.create(m.PdataVec3), sec.create(m.PdataReal), sec.create(m.PdataVec3)
    scale = 4.0 / max(flags.sx, flags.sy, flags.sz)
    m.resetSecondaryParticleStreams()

    def levelset():
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phi)

    def potentials(radius):
        m.flipComputeSecondaryParticlePotentials(pots[0], pots[1], pots[2], pots[3], flags, vel, normal, phi, radius, *PAR["taus"], scale)

    def one_pass(passes, radius=2):
        sv, sn, sc = _scratch_grid(s, m.VecGrid), _scratch_grid(s, m.VecGrid), _scratch_grid(s, m.IntGrid)
        f = lambda x: float(np.float32(x))
        s.lib.call("mf_secparts_potentials", flags.sx, flags.sy, flags.sz, pots[0].ptr, pots[1].ptr, pots[2].ptr, pots[3].ptr, flags.ptr, vel.ptr,
                   normal.ptr, phi.ptr, radius, *[f(t) for t in PAR["taus"]], f(scale), 1, 2 | 16 | 8, sv.ptr, sn.ptr, sc.ptr, passes, s.stream)

    spawned = []

    def sample():
        n0 = sec.pySize()
        m.flipSampleSecondaryParticles("single", flags, vel, sec, vSec, lSec, PAR["lMin"], PAR["lMax"], pots[0], pots[1], pots[2], pots[3],
                                       PAR["c_s"], PAR["c_b"], PAR["k_ta"], PAR["k_wc"])
        spawned.append(sec.pySize() - n0)

    def update():
        m.flipUpdateSecondaryParticles("linear", sec, vSec, lSec, fSec, flags, vel, pots[3], 1, PAR["gravity"], PAR["k_b"], PAR["k_d"], PAR["c_s"],
                                       PAR["c_b"], antitunneling=4)

    fns = [("potentials_r1", lambda: potentials(1)), ("potentials_r2", lambda: potentials(2)), ("pass_streaming", lambda: one_pass(1)),
           ("pass_gather_r2", lambda: one_pass(2)), ("partls_gather", lambda: m.averagedParticleLevelset(pp, pindex, flags, gpi, phi2, 1., 0, 0)),
           ("sample_single", sample), ("update_linear", update), ("delete_in_obstacle", lambda: m.flipDeleteParticlesInObstacle(sec, flags))]
    four = [fns[1][1], sample, update, fns[7][1]]
    ts = {k: [] for k, _ in fns}
    ts["step"], ts["step_with_secparts"] = [], []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    live = []
    for r in range(warmup + calls):
        levelset()
        for k, fn in fns:
            t = timed(fn)
            if r >= warmup:
                ts[k].append(t)
        live.append(sec.pySize())
        # the whole step without and with the four calls, alternated (the state moves on: both see the same stretch of the run)
        t_plain = timed(st["step"])
        levelset()
        t_with = timed(lambda: (st["step"](), [f() for f in four]))
        if r >= warmup:
            ts["step"].append(t_plain)
            ts["step_with_secparts"].append(t_with)
    n = flags.sx * flags.sy * flags.sz
    out = {"dims": [flags.sx, flags.sy, flags.sz], "particles": pp.pySize(), "warmup_calls": warmup, "timed_calls": calls,
           "spawned_per_sampling_call_median": int(np.median(spawned)), "secondary_slots_at_end": sec.pySize(),
           "secondary_live_at_end": int(((sec.get_flags() & (1 << 10)) == 0).sum())}
    for k, a in ts.items():
        a = np.asarray(a)
        out[k + "_ms"] = {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}
    pre = out["pass_streaming_ms"]["median"]
    out["streaming_pass_bytes"] = n * PRE_BYTES_PER_CELL
    out["streaming_pass_ms_at_hbm_peak"] = n * PRE_BYTES_PER_CELL / (HBM_PEAK_TBS * 1e12) * 1e3
    out["streaming_pass_fraction_of_hbm_peak"] = round(out["streaming_pass_ms_at_hbm_peak"] / pre, 3)
    out["gather_r2_to_partls_gather"] = round(out["pass_gather_r2_ms"]["median"] / out["partls_gather_ms"]["median"], 3)
    four_ms = sum(out[k + "_ms"]["median"] for k in ("potentials_r2", "sample_single", "update_linear", "delete_in_obstacle"))
    out["four_calls_ms"] = four_ms
    out["share_of_step_alternated"] = round(1.0 - out["step_ms"]["median"] / out["step_with_secparts_ms"]["median"], 3)
    return out


def kernel_stats(out_dir, warmup, calls):
    """the 128^3 calls alone in a child process under rocprofv3: the kernel table"""
    tmp = tempfile.mkdtemp(prefix="secparts_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--states", "flip01", "--warmup", str(warmup), "--calls", str(calls), "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        shutil.copyfile(found[0], os.path.join(out_dir, "secparts_kernel_stats.csv"))
        return True
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
        raise SystemExit("secparts_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "states": {}}
    for name in args.states.split(":"):
        st = {"flip01": flip01_state, "dam": dam_state}[name](m)
        torch.cuda.synchronize()
        out["states"][name] = time_state(m, torch, st, args.warmup, args.calls)
        del st
        torch.cuda.empty_cache()
    if stats:
        out["rocprofv3_flip01"] = "secparts_kernel_stats.csv"
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "secparts_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
