"""Per-call times of the fire, wave-equation and uv-grid plugins on one GPU: processBurn (without colours) at 128^3 and 256^3 against
its own bytes at the HBM peak (fuel, density, react read and written, heat written: 28 B per cell); extrapolateSimpleFlags(distance=6)
at 128^3 into an obstacle block deeper than six cells, per pass (the call has one mark launch and six pass launches; the figure is the
call's time over seven launches); cgSolveWE at 1024 x 1024 and 128^3 with its iteration count; normalizeSumTo at 256^3.  Every timed
window ends in a device synchronise; medians of --calls calls after --warmup.  Nothing exists at the parent commit to compare with.
Prints one JSON line and writes it to <out>/fields_time.json; with --stats, a child process first runs the 128^3 calls alone under
`rocprofv3 --kernel-trace --stats` (a run of its own) and its kernel table becomes <out>/fields_kernel_stats.csv.

  python tools/fields_time.py [--warmup 5] [--calls 10] [--out profiles] [--stats]
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
BURN_BYTES_PER_CELL = 3 * 8 + 4


def measure(warmup, calls, sizes):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fields_time.py needs a GPU")
    import manta as m

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median(fn, before=None):
        ts = []
        for q in range(warmup + calls):
            if before:
                before()
            t = timed(fn)
            if q >= warmup:
                ts.append(t)
        a = np.asarray(ts)
        return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}

    def solver(dims, dt=0.9):
        s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
        s.timestep = dt
        return s

    def rand(s, lo, hi, seed):
        g = s.create(m.RealGrid)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        g.data.copy_((torch.rand(g.n, generator=gen) * (hi - lo) + lo).to(g.data.device))
        return g

    out = {"device": torch.cuda.get_device_name(0), "warmup_calls": warmup, "timed_calls": calls, "hbm_peak_TBs": HBM_PEAK_TBS}
    for res in sizes["burn"]:
        s = solver((res, res, res), 0.4)
        fuel0, dens0, react0 = rand(s, 0, 1.3, 1), rand(s, 0, 1, 2), rand(s, 0, 1, 3)
        fuel, dens, react, heat = (s.create(m.RealGrid) for _ in range(4))
        r = median(lambda: m.processBurn(fuel=fuel, density=dens, react=react, heat=heat),
                   lambda: (fuel.copyFrom(fuel0), dens.copyFrom(dens0), react.copyFrom(react0)))
        nbytes = BURN_BYTES_PER_CELL * res ** 3
        r.update(bytes=nbytes, achieved_TBs=nbytes / (r["median_ms"] * 1e-3) / 1e12)
        r["share_of_hbm_peak"] = r["achieved_TBs"] / HBM_PEAK_TBS
        out["processBurn_%d" % res] = r
        del fuel0, dens0, react0, fuel, dens, react, heat, s
    res = sizes["extrap"]
    s = solver((res, res, res))
    flags, val0, val = s.create(m.FlagGrid), rand(s, -3, 3, 4), s.create(m.RealGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    f = flags.to_numpy()
    c = res // 2
    f[c - res // 4:c + res // 4, c - res // 4:c + res // 4, c - res // 4:c + res // 4] = 2
    flags.from_numpy(f)
    r = median(lambda: m.extrapolateSimpleFlags(flags=flags, val=val, distance=6), lambda: val.copyFrom(val0))
    r.update(dims=[res] * 3, launches=7, per_launch_ms=r["median_ms"] / 7)
    out["extrapolateSimpleFlags_d6_%d" % res] = r
    del flags, val0, val, s
    for dims in sizes["cg"]:
        s = solver(dims, 3.0)
        flags = s.create(m.FlagGrid)
        flags.initDomain()
        flags.fillGrid()
        ut0, utm10 = rand(s, -1, 1, 5), rand(s, -1, 1, 6)
        ut, utm1, o = (s.create(m.RealGrid) for _ in range(3))
        r = median(lambda: m.cgSolveWE(flags=flags, ut=ut, utm1=utm1, out=o, cSqr=0.9), lambda: (ut.copyFrom(ut0), utm1.copyFrom(utm10)))
        r.update(dims=list(dims), iterations=m.lastCgStats()["iterations"])
        out["cgSolveWE_%s" % "x".join(str(d) for d in dims)] = r
        del flags, ut0, utm10, ut, utm1, o, s
    res = sizes["normalize"]
    s = solver((res, res, res))
    h0, h = rand(s, -1, 3, 7), s.create(m.RealGrid)
    r = median(lambda: m.normalizeSumTo(h, 3.5), lambda: h.copyFrom(h0))
    r.update(dims=[res] * 3)
    out["normalizeSumTo_%d" % res] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:       # under rocprofv3: the 128^3 calls alone, a few times
        measure(1, 3, dict(burn=(128,), extrap=128, cg=((128, 128, 128),), normalize=128))
        return
    os.makedirs(a.out, exist_ok=True)
    if a.stats:
        tmp = tempfile.mkdtemp(prefix="fields_stats_")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"],
                       check=True, timeout=240, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if found:
            shutil.copy(found[0], os.path.join(a.out, "fields_kernel_stats.csv"))
        shutil.rmtree(tmp, ignore_errors=True)
    out = measure(a.warmup, a.calls, dict(burn=(128, 256), extrap=128, cg=((1024, 1024, 1), (128, 128, 128)), normalize=256))
    line = json.dumps(out)
    print(line)
    with open(os.path.join(a.out, "fields_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
