"""Per-call times of the grid operations (include/open/manta_hip_gridops.h) beside the yardsticks that existed before them, on one GPU
at 256^3.  Prints one JSON line and writes it to <out>/gridops_time.json.

  permuteAxes, the four permutations that move x (LDS tile) and the y<->z row-copy form, each beside Grid.copyFrom (mf_copy_f32) over the
      same bytes: a Real grid read once and written once.  permuteAxes is timed whole: one launch and a pointer swap.
  getL2 beside getMaxAbs on the same Real grid: both read the grid once and end in one scalar read-back, so both are host clocks around
      a call that synchronises.

Times: the median of 10 calls after 5 warm-up calls, with the minimum and maximum; the device times stand between two device events.
Each ratio is median / median with the range min / max .. max / min.  No ratio was fixed in advance: nothing had been measured.

  flipComputePotentialTrappedAir at radius 2 beside k_secparts_gather alone on the same grid (mf_secparts_potentials with passes = 2,
      after one run of its streaming pass has filled the scratch the gather reads), and beside the whole combined plugin for context.

The working set of the copy and of the permutations is 134 MB at 256^3 and fits the 256 MB Infinity Cache: those rates are cache-resident
rates, not HBM bandwidth, and the JSON says so (`cache_resident`).

  python tools/gridops_time.py [--n 256] [--out profiles]      (another n writes gridops_time_<n>.json; 512 leaves the cache: 1 GB)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 5, 10
PERMUTATIONS = {"x<->y (1,0,2)": (1, 0, 2), "x<->z (2,1,0)": (2, 1, 0), "cycle (1,2,0)": (1, 2, 0), "cycle (2,0,1)": (2, 0, 1),
                "y<->z row copy (0,2,1)": (0, 2, 1)}


def stats(ts):
    ts = sorted(ts)
    return dict(median_us=round(ts[len(ts) // 2], 2), min_us=round(ts[0], 2), max_us=round(ts[-1], 2))


def ratio(a, b):
    return dict(median=round(a["median_us"] / b["median_us"], 3), min=round(a["min_us"] / b["max_us"], 3), max=round(a["max_us"] / b["min_us"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    import manta as m
    n = a.n
    s = m.Solver(name="t", gridSize=m.vec3(n, n, n), dim=3)
    g, h = s.create(m.RealGrid), s.create(m.RealGrid)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    g.data.copy_(torch.rand(g.data.numel(), device="cuda", generator=gen) * 2 - 1)

    def device_time(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(REPS):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return stats(ts)

    def host_time(fn):
        for _ in range(WARMUP):
            fn()
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        return stats(ts)

    res = dict(n=n, bytes_moved=8 * g.n, warmup=WARMUP, reps=REPS, device=torch.cuda.get_device_name(0),
               cache_resident=bool(8 * g.n < 256 << 20))      # source + target below the 256 MB Infinity Cache: not an HBM rate
    copy = device_time(lambda: h.copyFrom(g))
    copy["GBps"] = round(8 * g.n / copy["median_us"] / 1e3, 1)
    res["copy (mf_copy_f32)"] = copy
    res["permuteAxes"] = {}
    for name, ax in PERMUTATIONS.items():
        t = device_time(lambda: g.permuteAxes(*ax))
        t["GBps"] = round(8 * g.n / t["median_us"] / 1e3, 1)
        t["over_copy"] = ratio(t, copy)
        res["permuteAxes"][name] = t
    l2, mx = host_time(g.getL2), host_time(g.getMaxAbs)
    l2["over_getMaxAbs"] = ratio(l2, mx)
    res["getL2"], res["getMaxAbs"] = l2, mx
    # the trapped-air gather at radius 2 beside the combined plugin (k_secparts_pre + k_secparts_gather) on the same grid: fluid in the
    # lower half of a walled box, three cells from every side
    flags, vel, normal, phi = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.VecGrid), s.create(m.LevelsetGrid)
    pots = [s.create(m.RealGrid) for _ in range(4)]
    flags.initDomain(boundaryWidth=0)
    flags._view()[3:-3, 3:n // 2, 3:-3] = m.FlagFluid
    for t in (vel, normal):
        t.data.copy_(torch.rand(t.data.numel(), device="cuda", generator=gen) * 2 - 1)
    phi.data.copy_(torch.rand(phi.data.numel(), device="cuda", generator=gen) * 2 - 1)
    ta = device_time(lambda: m.flipComputePotentialTrappedAir(pots[0], flags, vel, 2, 0.1, 1.0, 1.0 / n))
    both = device_time(lambda: m.flipComputeSecondaryParticlePotentials(pots[0], pots[1], pots[2], pots[3], flags, vel, normal, phi, 2, 0.1, 1.0, 0.1,
                                                                        1.0, 0.1, 1.0, 1.0 / n, m.FlagFluid, m.FlagObstacle))
    from mantaflow_amd.core import _ptr
    sv, sn, sc = s.create(m.VecGrid), s.create(m.VecGrid), s.create(m.IntGrid)

    def secparts(passes):
        s.lib.call("mf_secparts_potentials", n, n, n, pots[0].ptr, pots[1].ptr, pots[2].ptr, pots[3].ptr, flags.ptr, vel.ptr, normal.ptr, phi.ptr,
                   2, 0.1, 1.0, 0.1, 1.0, 0.1, 1.0, 1.0 / n, m.FlagFluid, m.FlagObstacle, sv.ptr, sn.ptr, _ptr(sc.data), passes, s.stream)
    secparts(1)
    gather = device_time(lambda: secparts(2))
    ta["over_k_secparts_gather"] = ratio(ta, gather)
    ta["over_combined"] = ratio(ta, both)
    res["flipComputePotentialTrappedAir r=2"] = ta
    res["k_secparts_gather r=2 (mf_secparts_potentials, passes = 2)"] = gather
    res["flipComputeSecondaryParticlePotentials r=2 (k_secparts_pre + k_secparts_gather)"] = both
    line = json.dumps(res)
    print(line)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "gridops_time.json" if n == 256 else "gridops_time_%d.json" % n), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
