"""Per-call times of the array bridge and the MLFLIP data plugins on one GPU, on two liquid states: scenes/flip01_simple.py's loop at
128^3 (bench.py's config 3) and scenes/benchmark_dam.py's at 379x356x124 (bench.py's config 4), each a few steps into its run.

  features   extractFeatureVel + Phi + Geo with window 1 into one matrix of 135 columns, into a tensor on the device and into a numpy
             array (alternated); the particles are sub-sampled (every k-th) where the matrix would pass 2 GB.  Yardstick: the bytes of the
             matrix written once at the HBM peak; the host form moves the matrix over the host link twice per call on top
  vec copies copyGridToArrayMAC / copyArrayToGridMAC with a float32 tensor on the device (12 bytes read and 12 written per cell) against
             the HBM peak, and with a numpy array
  regions    getRegions, getRegionalCounts and extendRegion(depth=1) on the state's flags (ctype fluid), with the region count; yardstick:
             flags read once and the result written once (8 bytes per cell)

Medians (with min and max) of --calls calls after --warmup; every timed window ends in a device synchronise.  Nothing exists at the parent
commit to compare with.  Prints one JSON line and writes it to <out>/mlflip_time.json; with --stats, a child process first runs the
128^3 calls under `rocprofv3 --kernel-trace --stats` (a run of its own) and its kernel table becomes <out>/mlflip_kernel_stats.csv.

  python tools/mlflip_time.py [--warmup 5] [--calls 10] [--states flip01:dam] [--out profiles] [--stats]
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
MATRIX_LIMIT = 2 * 10 ** 9    # bytes of the feature matrix above which the particles are sub-sampled
FLUID, OBSTACLE, EMPTY = 1, 2, 4


def flip01_state(m, n=128, steps=3):
    """bench.py's config 3 (flip01_simple.py's loop, 8 particles per cell in the lower 0.4 x 0.6 x 1.0 block), `steps` steps in"""
    s = m.Solver(name="flip01", gridSize=m.vec3(n, n, n), dim=3)
    s.timestep = 0.5
    flags, phi = s.create(m.FlagGrid), s.create(m.LevelsetGrid)
    flags.initDomain(boundaryWidth=0)
    flags.updateFromLevelset(m.Box(parent=s, p0=m.vec3(0, 0, 0), p1=m.vec3(0.4 * n, 0.6 * n, n)).computeLevelset())
    pp = s.create(m.BasicParticleSystem)
    m.sampleFlagsWithParticles(flags, pp, 2, 0.2)
    pv = pp.create(m.PdataVec3)
    vel, velOld, w, pres = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.RealGrid)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    for _ in range(steps):
        pp.advectInGrid(flags, vel, 2, deleteInObstacle=False)
        m.mapPartsToMAC(flags, vel, velOld, pp, pv, w)
        m.extrapolateMACFromWeight(vel, w, distance=2)
        m.markFluidCells(pp, flags)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phi)
        m.addGravity(flags, vel, m.vec3(0, -0.002, 0))
        m.setWallBcs(flags, vel)
        m.solvePressure(vel, pres, flags)
        m.extrapolateMACSimple(flags, vel)
        m.flipVelocityUpdate(flags, vel, velOld, pp, pv, 0.97)
        s.step()
    return dict(s=s, flags=flags, parts=pp, vel=vel, phi=phi, keep=(pv, velOld, w, pres, pindex, gpi))


def dam_state(m, steps=4):
    """bench.py's config 4 (benchmark_dam.py at res 116: 379 x 356 x 124), `steps` steps in"""
    import bench
    from mantaflow_amd import core, plugins, scene
    sc = bench.dam_scene(core, plugins, scene, bench.DAM_RES)
    for _ in range(steps):
        sc["step"]()
    return dict(s=sc["s"], flags=sc["flags"], parts=sc["parts"], vel=sc["vel"], phi=sc["phi"], keep=sc)


def time_state(m, torch, st, warmup, calls):
    import numpy as np
    s, flags, pp, vel, phi = st["s"], st["flags"], st["parts"], st["vel"], st["phi"]
    n_cells = flags.n

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def alternated(fns):
        """{name: fn} -> {name: stats}; the calls take turns so that they see the same machine state"""
        ts, last = {k: [] for k in fns}, {}
        for r in range(warmup + calls):
            for k, fn in fns.items():
                t, last[k] = timed(fn)
                if r >= warmup:
                    ts[k].append(t)
        out = {}
        for k, v in ts.items():
            a = np.asarray(v)
            out[k] = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}
        return out, last

    def against_peak(r, nbytes):
        r.update(bytes=int(nbytes), achieved_TBs=nbytes / (r["median_ms"] * 1e-3) / 1e12)
        r["share_of_hbm_peak"] = r["achieved_TBs"] / HBM_PEAK_TBS

    out = {"dims": [flags.sx, flags.sy, flags.sz], "particles": pp.pySize(), "warmup_calls": warmup, "timed_calls": calls}

    # features: window 1, one matrix for the three plugins
    window, nst = 1, 27
    N_row = 5 * nst
    every = max(1, -(-pp.pySize() * N_row * 4 // MATRIX_LIMIT))
    sub = pp
    if every > 1:
        sub = s.create(m.BasicParticleSystem)
        sub.resizeAll(len(range(0, pp.pySize(), every)))
        for c in range(3):
            sub.pos[c * sub.cap:c * sub.cap + sub.np] = pp.pos[c * pp.cap:c * pp.cap + pp.np][::every]
        sub.flag[:sub.np] = pp.flag[:pp.np][::every]
    n = sub.pySize()

    def features(fv):
        m.extractFeatureVel(fv, N_row, 0, sub, vel, 1.0, None, 0, window)
        m.extractFeaturePhi(fv, N_row, 3 * nst, sub, phi, 1.0, None, 0, window)
        m.extractFeatureGeo(fv, N_row, 4 * nst, sub, flags, 1.0, None, 0, window)

    fv_dev = torch.zeros(n * N_row, dtype=torch.float32, device=s.device)
    fv_host = np.zeros(n * N_row, np.float32)
    r, _ = alternated({"device_tensor": lambda: features(fv_dev), "numpy_array": lambda: features(fv_host)})
    against_peak(r["device_tensor"], 4 * n * N_row)
    r["numpy_array"]["bytes_over_host_link"] = int(3 * 2 * 4 * n * N_row)       # each of the three calls uploads and downloads the matrix
    r.update(particles_used=n, every=every, columns=N_row, matrix_bytes=int(4 * n * N_row),
             host_over_device=r["numpy_array"]["median_ms"] / r["device_tensor"]["median_ms"])
    assert bool((torch.from_numpy(fv_host) == fv_dev.cpu()).all()), "the two forms differ"
    out["features_window1"] = r
    del fv_dev, fv_host

    # the vector copies
    a_dev = torch.zeros((flags.sz, flags.sy, flags.sx, 3), dtype=torch.float32, device=s.device)
    a_host = np.zeros((flags.sz, flags.sy, flags.sx, 3), np.float32)
    tmp = s.create(m.MACGrid)
    r, _ = alternated({"grid_to_device_tensor": lambda: m.copyGridToArrayMAC(vel, a_dev), "device_tensor_to_grid": lambda: m.copyArrayToGridMAC(a_dev, tmp),
                       "grid_to_numpy": lambda: m.copyGridToArrayMAC(vel, a_host), "numpy_to_grid": lambda: m.copyArrayToGridMAC(a_host, tmp)})
    for k in ("grid_to_device_tensor", "device_tensor_to_grid"):
        against_peak(r[k], 24 * n_cells)
    out["copy_mac_float32"] = r
    del a_dev, a_host, tmp

    # regions and flags
    work, rg = s.create(m.FlagGrid), s.create(m.IntGrid)
    work.copyFrom(flags)

    def extend():
        work.copyFrom(flags)
        m.extendRegion(work, EMPTY, OBSTACLE, 1)

    r, last = alternated({"getRegions": lambda: m.getRegions(rg, flags, FLUID), "getRegionalCounts": lambda: m.getRegionalCounts(rg, flags, FLUID),
                          "extendRegion_depth1_with_flag_copy": extend, "flag_copy_alone": lambda: work.copyFrom(flags)})
    for k in ("getRegions", "getRegionalCounts", "extendRegion_depth1_with_flag_copy"):
        against_peak(r[k], 8 * n_cells)
    r["regions"] = int(last["getRegions"])
    r["fluid_cells"] = int((flags.data & FLUID).ne(0).sum().item())
    out["regions_fluid"] = r
    return out


def kernel_stats(out_dir):
    tmp = tempfile.mkdtemp(prefix="mlflip_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--states", "flip01", "--warmup", "1", "--calls", "2", "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        shutil.copyfile(found[0], os.path.join(out_dir, "mlflip_kernel_stats.csv"))
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
    if args.stats:
        kernel_stats(args.out)                     # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mlflip_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_TBs": HBM_PEAK_TBS, "states": {}}
    for name in args.states.split(":"):
        st = {"flip01": flip01_state, "dam": dam_state}[name](m)
        torch.cuda.synchronize()
        out["states"][name] = time_state(m, torch, st, args.warmup, args.calls)
        del st
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "mlflip_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
