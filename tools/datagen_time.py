"""Per-call times of the smoke data-generation plugins on one GPU, on a 128^3 and a 256^3 smoke state (the 256^3 one is the fine grid
of tensorflow/example3_resnet/manta_genSimData2.py at res 64, scale 4, with its blur sigma 4 / 3.544908 = 1.128: 7 taps).  A state is
a density from three densityInflow sources and a velocity from three initial-velocity spheres, blurred once; no solver step is taken
(none of the timed kernels depends on the values).

  blurs       blurRealGrid and blurMacGrid, out of place; yardstick: every pass streams its grid once in and once out at the HBM peak
              (8 B per cell and pass for a real grid, 24 B for a MAC grid); beside them mf_guiding_blur at radius 3 (7 taps as well) on
              the same MAC grid
  projection  projectImage in smoke mode and in surface mode, and the three views one at a time (image clear, one view's kernel, the
              read-back of the whole image); yardstick: one read of the grid (4 B per cell)
  reductions  calcCenterOfMass against one read of the grid
  stencils    getLaplacian and getCurvature against 8 B per cell

Medians (with min and max) of --calls calls after --warmup, alternated within a group; every timed window ends in a device
synchronise.  Nothing exists at the parent commit to compare with.  Prints one JSON line and writes it to <out>/datagen_time.json;
with --stats, a child process first runs the calls under `rocprofv3 --kernel-trace --stats` (a run of its own), its kernel table
becomes <out>/datagen_kernel_stats.csv and the rows of this extension's kernels are added to the JSON (per-pass and per-view times).

  python tools/datagen_time.py [--warmup 5] [--calls 10] [--sizes 128:256] [--out profiles] [--stats]
"""
import argparse
import csv
import ctypes
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
BLUR_SIGMA = 4.0 / 3.544908   # the scripts' value for scale 4


def smoke_state(m, n):
    s = m.Solver(name="smoke%d" % n, gridSize=m.vec3(n, n, n), dim=3)
    flags, density, vel = s.create(m.FlagGrid), s.create(m.RealGrid), s.create(m.MACGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    for q, (c, r) in enumerate((((0.5, 0.3, 0.5), 0.14), ((0.35, 0.55, 0.6), 0.1), ((0.65, 0.6, 0.4), 0.12))):
        noise = s.create(m.NoiseField, fixedSeed=100 + q, loadFromFile=True)
        noise.posScale, noise.clamp, noise.clampNeg, noise.clampPos = m.vec3(n * 0.15), True, 0, 1.0
        noise.valScale, noise.valOffset, noise.timeAnim = 1.0, 0.2, 0.3
        m.densityInflow(flags=flags, density=density, noise=noise, shape=s.create(m.Sphere, center=m.vec3(c[0] * n, c[1] * n, c[2] * n), radius=r * n), scale=1.0, sigma=1.0)
    for c, r, v in (((0.4, 0.4, 0.5), 0.1, (0.8, -0.5, 0.3)), ((0.6, 0.5, 0.45), 0.08, (-0.6, 0.4, -0.2)), ((0.5, 0.65, 0.55), 0.12, (0.2, 0.7, 0.5))):
        s.create(m.Sphere, center=m.vec3(c[0] * n, c[1] * n, c[2] * n), radius=r * n).applyToGrid(grid=vel, value=m.vec3(*v))
    m.blurMacGrid(vel, vel, BLUR_SIGMA)
    return dict(s=s, flags=flags, density=density, vel=vel)


def time_state(m, torch, st, warmup, calls):
    import numpy as np
    from mantaflow_amd import plugins
    s, flags, density, vel = st["s"], st["flags"], st["density"], st["vel"]
    n_cells = flags.n

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def alternated(fns, peak_bytes=None):
        """{name: fn} -> {name: stats}; the calls take turns so that they see the same machine state"""
        ts = {k: [] for k in fns}
        for r in range(warmup + calls):
            for k, fn in fns.items():
                t, _ = timed(fn)
                if r >= warmup:
                    ts[k].append(t)
        out = {}
        for k, v in ts.items():
            a = np.asarray(v)
            out[k] = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}
            nbytes = (peak_bytes or {}).get(k)
            if nbytes:
                out[k].update(bytes=int(nbytes), achieved_TBs=nbytes / (out[k]["median_ms"] * 1e-3) / 1e12)
                out[k]["share_of_hbm_peak"] = out[k]["achieved_TBs"] / HBM_PEAK_TBS
        return out

    out = {"dims": [flags.sx, flags.sy, flags.sz], "warmup_calls": warmup, "timed_calls": calls, "sigma": BLUR_SIGMA}

    # blurs; the guiding blur at radius 3 beside them
    realT, macT, work = s.create(m.RealGrid), s.create(m.MACGrid), s.create(m.MACGrid)
    s1, s2 = s.create(m.MACGrid), s.create(m.MACGrid)
    w = np.zeros(7, np.float32)
    s.lib.call("mf_guiding_weights", 3, w.ctypes.data_as(ctypes.c_void_p))
    w_dev = torch.from_numpy(w).to(s.device)
    work.copyFrom(vel)

    def guiding():
        s.lib.call("mf_guiding_blur", flags.sx, flags.sy, flags.sz, flags.ptr, work.ptr, s1.ptr, s2.ptr, ctypes.c_void_p(w_dev.data_ptr()), 3, 1, s.stream)

    out["mdim"] = m.blurRealGrid(density, realT, BLUR_SIGMA)
    out["blur"] = alternated({"blurRealGrid": lambda: m.blurRealGrid(density, realT, BLUR_SIGMA), "blurMacGrid": lambda: m.blurMacGrid(vel, macT, BLUR_SIGMA),
                              "mf_guiding_blur_radius3": guiding},
                             {"blurRealGrid": 3 * 8 * n_cells, "blurMacGrid": 3 * 24 * n_cells, "mf_guiding_blur_radius3": 3 * 24 * n_cells})
    out["blur"]["blurMacGrid_over_guiding"] = out["blur"]["blurMacGrid"]["median_ms"] / out["blur"]["mf_guiding_blur_radius3"]["median_ms"]
    del realT, macT, work, s1, s2

    # projection
    view = lambda mode, v: (lambda: plugins._project("projectImage", density, mode, 1.0, views=v))
    fns = {"projectImage_smoke": lambda: m.projectImage(density, 0, 1.0), "projectImage_surfaces": lambda: m.projectImage(density, 1, 1.0)}
    for mode, tag in ((0, "smoke"), (1, "surfaces")):
        for v, axis in ((1, "z"), (2, "x"), (4, "y")):
            fns["view_%s_%s" % (axis, tag)] = view(mode, v)
    fns["no_view_clear_and_read_back"] = view(0, 0)
    out["projection"] = alternated(fns, {k: 4 * n_cells for k in fns if k.startswith("view_")})
    out["projection"]["image_bytes"] = int(3 * (3 * flags.sx) * flags.sx)

    # the reduction and the stencils
    lap, curv = s.create(m.RealGrid), s.create(m.RealGrid)
    out["reduction_and_stencils"] = alternated(
        {"calcCenterOfMass": lambda: m.calcCenterOfMass(density), "getLaplacian": lambda: m.getLaplacian(lap, density),
         "getCurvature": lambda: m.getCurvature(curv, density, 0.5)},
        {"calcCenterOfMass": 4 * n_cells, "getLaplacian": 8 * n_cells, "getCurvature": 8 * n_cells})
    return out


def kernel_stats(out_dir, sizes):
    """the traced child's kernel table, copied to out_dir; returns the rows of this extension's kernels"""
    tmp = tempfile.mkdtemp(prefix="datagen_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--sizes", sizes, "--warmup", "1", "--calls", "3", "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        dst = os.path.join(out_dir, "datagen_kernel_stats.csv")
        shutil.copyfile(found[0], dst)
        with open(dst) as f:
            return [row for row in csv.DictReader(f) if "datagen" in row.get("Name", "")]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sizes", default="128:256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the largest size (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sizes = [int(v) for v in args.sizes.split(":")]
    rows = kernel_stats(args.out, str(max(sizes))) if args.stats else None      # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("datagen_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_TBs": HBM_PEAK_TBS, "states": {}}
    for n in sizes:
        st = smoke_state(m, n)
        torch.cuda.synchronize()
        out["states"]["%d^3" % n] = time_state(m, torch, st, args.warmup, args.calls)
        del st
        torch.cuda.empty_cache()
    if rows is not None:
        out["kernels_traced_at_%d^3" % max(sizes)] = rows
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "datagen_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
