"""Per-call times of the turbulence model on the state of tools/tests/test_2025_turb.py's loop at 128 x 64 x 64 and 256 x 128 x 128,
a few steps in: the four k-epsilon plugins; advectInGrid, synthesize (one octave) and deleteInObstacle of a turbulence particle system
of 100 k and 1 M particles; the fused production kernel against its own bytes (vel 12 + k 4 + eps 4 read, k, eps, prod, nuT, strain
20 written: 40 B per cell) at the HBM peak; KEpsilonGradientDiffusion (three fused launches) alternated with a chain of the package's
per-operation grid methods -- the package has no stand-alone LaplaceOp, so the chain uses copyFrom in its place and is a LOWER bound
of the composed form: per field copyFrom, mult(nuT), multConst, add, and getComponent / setComponent around it for the velocity;
synthesize per curl evaluation against applyNoiseVec3 per cell on the same tile; and the turbulence calls' share of the whole step,
from per-call windows inside the loop.  Every timed window ends in a device synchronise; medians of --calls calls after --warmup.
Prints one JSON line and writes it to <out>/turbulence_time.json; with --stats, a child process first runs the 128 x 64 x 64 calls
alone under `rocprofv3 --kernel-trace --stats` and its kernel table becomes <out>/turbulence_kernel_stats.csv.

  python tools/turbulence_time.py [--warmup 5] [--calls 10] [--res 128:256] [--out profiles] [--stats]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_TBS = 8.0            # MI355X HBM3E peak, the figure the README's other sections use
PRODUCTION_BYTES_PER_CELL = 12 + 4 + 4 + 20


def time_state(m, torch, M, res, warmup, calls, steps_in=4):
    import numpy as np
    m.resetTurbulenceParticleState()
    g = M.setup_loop_pkg(m, res, 1.2)
    for _ in range(steps_in):
        M.step_loop_pkg(m, g)
    s, flags, vel, k, eps = g["s"], g["flags"], g["vel"], g["k"], g["eps"]
    n = flags.sx * flags.sy * flags.sz

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stat(a):
        a = np.asarray(a)
        return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}

    out = {"dims": [flags.sx, flags.sy, flags.sz], "warmup_calls": warmup, "timed_calls": calls}
    # ---- the plugins on copies of the state (so that repeated calls see the same numbers)
    kc, ec, vc, tmp, comp = s.create(m.RealGrid), s.create(m.RealGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.RealGrid)
    noise_target = s.create(m.VecGrid)

    def restore():
        kc.copyFrom(k), ec.copyFrom(eps), vc.copyFrom(vel)

    def composed():
        dt = float(np.float32(s.getDt()))
        for f, sigma in ((kc, 1.0), (ec, 1.3)):
            tmp.copyFrom(f), tmp.mult(g["nuT"]), tmp.multConst(dt / sigma), f.add(tmp)
        for c in range(3):
            m.getComponent(vc, comp, c)
            tmp.copyFrom(comp), tmp.mult(g["nuT"]), tmp.multConst(dt / 10.0), comp.add(tmp)
            m.setComponent(comp, vc, c)

    fns = [("KEpsilonBcs", lambda: m.KEpsilonBcs(flags=flags, k=kc, eps=ec, intensity=0.1, nu=0.1, fillArea=False)),
           ("KEpsilonComputeProduction", lambda: m.KEpsilonComputeProduction(vel=vel, k=kc, eps=ec, prod=g["prod"], nuT=g["nuT"], strain=g["strain"], pscale=2.5)),
           ("KEpsilonSources", lambda: m.KEpsilonSources(k=kc, eps=ec, prod=g["prod"])),
           ("KEpsilonGradientDiffusion", lambda: m.KEpsilonGradientDiffusion(k=kc, eps=ec, vel=vc, nuT=g["nuT"], sigmaU=10.0)),
           ("graddiff_composed_lower_bound", composed),
           ("applyNoiseVec3", lambda: m.applyNoiseVec3(flags, noise_target, g["turb"].noise, scale=0.1, scaleSpatial=1.0))]
    ts = {name: [] for name, _ in fns}
    for r in range(warmup + calls):
        for name, fn in fns:               # alternated: every round runs each form once
            restore()
            t = timed(fn)
            if r >= warmup:
                ts[name].append(t)
    for name in ts:
        out[name + "_ms"] = stat(ts[name])
    p = out["KEpsilonComputeProduction_ms"]["median"]
    out["production_bytes"] = n * PRODUCTION_BYTES_PER_CELL
    out["production_ms_at_hbm_peak"] = n * PRODUCTION_BYTES_PER_CELL / (HBM_PEAK_TBS * 1e12) * 1e3
    out["production_fraction_of_hbm_peak"] = round(out["production_ms_at_hbm_peak"] / p, 3)
    out["production_note"] = "repeated calls on the same grids: a warm-cache figure where the %d MB working set fits the 256 MB last-level cache" % (
        n * PRODUCTION_BYTES_PER_CELL // 2 ** 20)
    ratios = np.asarray(ts["graddiff_composed_lower_bound"]) / np.asarray(ts["KEpsilonGradientDiffusion"])
    out["graddiff_composed_lower_bound_over_fused"] = stat(ratios)
    fluid = int(((flags.to_numpy() & 1) != 0).sum())
    out["applyNoiseVec3_ns_per_curl"] = out["applyNoiseVec3_ms"]["median"] * 1e6 / fluid
    # ---- the particle calls at two sizes: a box across the inflow half of the domain
    gs = g["gs"]
    box = m.Box(parent=s, center=gs * m.vec3(0.3, 0.5, 0.5), size=gs * m.vec3(0.2, 0.4, 0.4))
    for npart in (100000, 1000000):
        turb = s.create(m.TurbulenceParticleSystem, noise=g["turb"].noise)
        turb.seed(box, npart)
        pts = {"advectInGrid": [], "synthesize": [], "deleteInObstacle": []}
        for r in range(warmup + calls):
            for name, fn in (("advectInGrid", lambda: turb.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4)),
                             ("synthesize", lambda: turb.synthesize(flags=flags, octaves=1, k=k, switchLength=5, L0=0.01, scale=0.1)),
                             ("deleteInObstacle", lambda: turb.deleteInObstacle(flags))):
                t = timed(fn)
                if r >= warmup:
                    pts[name].append(t)
        key = "particles_%d" % npart
        out[key] = {name + "_ms": stat(a) for name, a in pts.items()}
        out[key]["slots_at_end"] = turb.pySize()
        out[key]["synthesize_ns_per_curl"] = out[key]["synthesize_ms"]["median"] * 1e6 / (2 * max(turb.pySize(), 1))     # n0 and n1, one octave
        del turb
    # ---- the turbulence calls' share of the step: per-call windows inside the loop
    shares = []
    for r in range(warmup + calls):
        acc = {}

        def timer(name, fn):
            acc[name] = acc.get(name, 0.0) + timed(fn)
        total = timed(lambda: M.step_loop_pkg(m, g, timer))
        if r >= warmup:
            shares.append((sum(acc.values()), total))
    out["step_ms"] = stat([t for _, t in shares])
    out["turbulence_calls_ms_in_step"] = stat([a for a, _ in shares])
    out["turbulence_share_of_step"] = stat([a / t for a, t in shares])
    out["loop_particles_at_end"] = g["turb"].pySize()
    return out


def kernel_stats(out_dir, warmup, calls):
    """the 128 x 64 x 64 calls alone in a child process under rocprofv3: the kernel table"""
    tmp = tempfile.mkdtemp(prefix="turbulence_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--res", "128", "--warmup", str(warmup), "--calls", str(calls), "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        shutil.copyfile(found[0], os.path.join(out_dir, "turbulence_kernel_stats.csv"))
        return True
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--res", default="128:256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the 128 x 64 x 64 calls (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    stats = kernel_stats(args.out, args.warmup, args.calls) if args.stats else None       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("turbulence_time.py needs a GPU")
    import manta as m
    import turbulence_model as M
    out = {"gpu": torch.cuda.get_device_name(0), "states": {}}
    for res in args.res.split(":"):
        out["states"][res] = time_state(m, torch, M, int(res), args.warmup, args.calls)
        torch.cuda.empty_cache()
    if stats:
        out["rocprofv3_128"] = "turbulence_kernel_stats.csv"
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "turbulence_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
