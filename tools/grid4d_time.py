"""Per-call times of the 4-D grids and the particle-data sums on one GPU: interpolateGrid4d and interpolateGrid4dVec 40^4 -> 80^4 and
back, against their own bytes at the HBM peak (target written once, source read once); the nearest cell counts through the existing 3-D
interpolateGrid (137^3 -> 345^3 and back) as a second yardstick; setBoundNeumann and getMaxAbs at 80^4; PdataReal.sum and setNoisePdata at
1 M and 8 M particles (the noise tile, 8 MB, stays in cache).  Every timed window ends in a device synchronise; medians with min and max of --calls calls after --warmup.  Nothing exists
at the parent commit to compare with.  Working sets: a 40^4 Real grid is 10 MB and a 40^4 Vec4 grid 41 MB, both inside the 256 MB
last-level cache, so the source of the upward step is a warm-cache read; an 80^4 Real grid is 164 MB (inside it, when nothing else is)
and an 80^4 Vec4 grid 655 MB (outside).  Prints one JSON line and writes it to <out>/grid4d_time.json; with --stats, a child process
first runs the calls once under `rocprofv3 --kernel-trace --stats` (a run of its own) and its kernel table becomes
<out>/grid4d_kernel_stats.csv.

  python tools/grid4d_time.py [--warmup 5] [--calls 10] [--out profiles] [--stats]
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


def measure(warmup, calls, small, large, parts):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grid4d_time.py needs a GPU")
    import manta as m

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median(fn, nbytes=None):
        ts = [timed(fn) for _ in range(warmup + calls)][warmup:]
        a = np.asarray(ts)
        r = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}
        if nbytes:
            r.update(bytes=int(nbytes), achieved_TBs=nbytes / (r["median_ms"] * 1e-3) / 1e12)
            r["share_of_hbm_peak"] = r["achieved_TBs"] / HBM_PEAK_TBS
        return r

    def fill(g, seed):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        n = g.data.numel()
        g.data.copy_((torch.rand(min(n, 1 << 22), generator=gen) * 2 - 1).repeat((n + (1 << 22) - 1) >> 22)[:n].to(g.data.device))
        return g

    out = {"device": torch.cuda.get_device_name(0), "warmup_calls": warmup, "timed_calls": calls, "hbm_peak_TBs": HBM_PEAK_TBS}
    S = m.Solver(name="small", gridSize=m.vec3(small, small, small), dim=3, fourthDim=small)
    L = m.Solver(name="large", gridSize=m.vec3(large, large, large), dim=3, fourthDim=large)
    for cls, fn, nc, tag in ((m.Grid4Real, m.interpolateGrid4d, 1, "interpolateGrid4d"), (m.Grid4Vec4, m.interpolateGrid4dVec, 4, "interpolateGrid4dVec")):
        a, b = fill(S.create(cls), 1), fill(L.create(cls), 2)
        nbytes = 4 * nc * (small ** 4 + large ** 4)
        out["%s_%d_to_%d" % (tag, small, large)] = median(lambda: fn(target=b, source=a), nbytes)
        out["%s_%d_to_%d" % (tag, large, small)] = median(lambda: fn(target=a, source=b), nbytes)
        if nc == 1:
            r = median(lambda: b.setBoundNeumann(1))
            r.update(dims=[large] * 4)
            out["setBoundNeumann_%d" % large] = r
            r = median(lambda: b.getMaxAbs(), 4 * large ** 4)
            out["getMaxAbs_%d" % large] = r
        else:
            r = median(lambda: b.getMaxAbs(), 16 * large ** 4)
            out["getMaxAbs_vec4_%d" % large] = r
        del a, b
    s3, l3 = int(round(small ** (4 / 3.))), int(round(large ** (4 / 3.)))
    S3, L3 = m.Solver(name="s3", gridSize=m.vec3(s3, s3, s3), dim=3), m.Solver(name="l3", gridSize=m.vec3(l3, l3, l3), dim=3)
    a, b = fill(S3.create(m.RealGrid), 3), fill(L3.create(m.RealGrid), 4)
    nbytes = 4 * (s3 ** 3 + l3 ** 3)
    out["interpolateGrid_%d_to_%d" % (s3, l3)] = median(lambda: m.interpolateGrid(target=b, source=a), nbytes)
    out["interpolateGrid_%d_to_%d" % (l3, s3)] = median(lambda: m.interpolateGrid(target=a, source=b), nbytes)
    out["interpolateGrid_cells"] = {"small": s3 ** 3, "large": l3 ** 3, "small_4d": small ** 4, "large_4d": large ** 4}
    del a, b
    P = m.Solver(name="p", gridSize=m.vec3(64, 64, 64), dim=3)
    noise = P.create(m.NoiseField, fixedSeed=265)
    for n in parts:
        sys_ = P.create(m.BasicParticleSystem)
        pd = sys_.create(m.PdataReal)
        sys_.resizeAll(n)
        pd.data.copy_(torch.rand(n, generator=torch.Generator(device="cpu").manual_seed(5)).to(pd.data.device))
        out["PdataReal_sum_%d" % n] = median(lambda: pd.sum(), 4 * n)
        gen = torch.Generator(device="cpu").manual_seed(6)
        for c in range(3):
            sys_.pos[c * sys_.cap:c * sys_.cap + n] = (torch.rand(n, generator=gen) * 64).to(sys_.pos.device)
        out["setNoisePdata_%d" % n] = median(lambda: m.setNoisePdata(sys_, pd, noise), 16 * n)      # three position planes read, one value written
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:       # under rocprofv3: every call a few times
        measure(1, 2, 40, 80, (1 << 20,))
        return
    os.makedirs(a.out, exist_ok=True)
    if a.stats:
        tmp = tempfile.mkdtemp(prefix="grid4d_stats_")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"],
                       check=True, timeout=240, stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if found:
            shutil.copy(found[0], os.path.join(a.out, "grid4d_kernel_stats.csv"))
        shutil.rmtree(tmp, ignore_errors=True)
    out = measure(a.warmup, a.calls, 40, 80, (1 << 20, 1 << 23))
    line = json.dumps(out)
    print(line)
    with open(os.path.join(a.out, "grid4d_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
