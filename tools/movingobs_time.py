"""Per-call device times of the moving-obstacle and obstacle-coupling entries (include/open/manta_hip_movingobs.h) on one GPU, at 128^3
and 256^3: a walled box, fluid in the lower half, a sphere obstacle, random velocities, and for the particle projection one million
particles.  Prints one JSON line and writes it to <out>/movingobs_time.json.

Times: each call stands between two device events and the stream is synchronised before the events are read; the median and the
minimum of --reps calls after one warm-up call.  A time therefore holds the launch latency of its kernels, which is most of it for the
cheapest entries at 128^3.  BasicParticleSystem.projectOutside draws its random numbers on the host between its two kernels, so its
figure is a host clock around a call that ends in a synchronise.

Beside each time: `bytes`, the memory traffic the entry cannot avoid (the arrays every cell or particle reads or writes; stated per
entry in BYTES below -- conditional writes, such as the faces set_wall_bcs2 changes, are not counted), the rate that gives, and that
rate as a share of the copy bandwidth measured in the same run (MACGrid.copyFrom, the library's device copy, 24 B per cell) and of the
8 TB/s HBM peak.  bench.py reports no copy bandwidth of its own, so the yardstick is measured here, at the same sizes.  No threshold:
nothing had been measured for these kernels before.  setWallBcs, which has been on the device since the first release, is timed the
same way for context.

The two structural claims are counted, not timed (--count): child processes run K and 2K calls under `rocprofv3 --kernel-trace
--memory-copy-trace`, and the difference of the two traces over K is what one call launches and copies.  moveLinear must come to 2
kernel launches with one shape and with eight; BasicParticleSystem.projectOutside to one read-back (a device-to-host transfer of the
copy engine, or the runtime's own copy kernel, which is how it carries a few bytes into pinned host memory) beside the one upload of
the random numbers.

  python tools/movingobs_time.py [--reps 30] [--sizes 128:256] [--out profiles] [--count]
"""
import argparse
import collections
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

HBM_PEAK_TBS = 8.0
PARTICLES = 1000000
DISTANCE = 4
BYTES = {   # per cell (n) or per particle (np): what the entry must move
    "set_wall_bcs2": "4 n: the flags",
    "set_bound_MAC2_w1 / setBoundMAC_w1 / setBoundMAC_w1_normalOnly": "12 B per cell within 2 cells of a wall (the bands are 1 to 3 cells wide)",
    "mark_surface": "4 n: the flags (plus 4 B per cell whose TypeSurface bit changes)",
    "clear_obstacle": "4 n: the flags",
    "clamp_norm_real / clamp_norm_mac": "8 n / 24 n: every value read and, with val below every norm, written",
    "resetPhiInObs": "8 n: flags and sdf",
    "extrapolateMACSimple_phiObs": "3 (8 n + distance 4 n) passes + 16 n (phi, vel) + 24 n copy + 28 n into-boundary pass",
    "extrapolateMACSimple_plain": "the same without the 16 n",
    "moveLinear_1_shape / moveLinear_8_shapes": "8 n: the flags, once per pass",
    "obstacle_sign": "8 n", "gradient": "16 n",
    "projectOutside_particles": "68 np: 16 (pos, flag) + 4 (count) in the first kernel, 16 + 4 + 16 (reals) + 12 (pos) in the second; the gathers of the gradient come on top",
    "setWallBcs (context)": "28 n: flags, vel read and written",
    "copy (yardstick)": "24 n: a MAC grid read and written",
}


def scene(m, torch, n):
    s = m.Solver(name="t%d" % n, gridSize=m.vec3(n, n, n), dim=3)
    flags, vel, obvel, phi, phiObs, grad = (s.create(c) for c in (m.FlagGrid, m.MACGrid, m.MACGrid, m.LevelsetGrid, m.LevelsetGrid, m.VecGrid))
    flags.initDomain(boundaryWidth=0)
    v = flags._view()
    v[1:-1, 1:n // 2, 1:-1] = m.FlagFluid
    sphere = m.Sphere(parent=s, center=m.vec3(0.5 * n, 0.45 * n, 0.5 * n), radius=0.15 * n)
    sphere.applyToGrid(grid=flags, value=m.FlagObstacle)
    phiObs.copyFrom(sphere.computeLevelset())
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    for t in (vel, obvel, grad):
        t.data.copy_(torch.rand(t.data.numel(), device="cuda", generator=g) * 2 - 1)
    phi.data.copy_(torch.rand(phi.data.numel(), device="cuda", generator=g) * 2 - 1)
    return dict(s=s, n=n, flags=flags, vel=vel, obvel=obvel, phi=phi, phiObs=phiObs, grad=grad)


def obstacle(m, st, shapes):
    n, s = st["n"], st["s"]
    m.resetMovingObstacleState()
    mo = m.MovingObstacle(s)
    for q in range(shapes):
        mo.add(m.Sphere(parent=s, center=m.vec3(0.3 * n, 0.5 * n, 0.5 * n), radius=(0.05 + 0.01 * q) * n) if q % 2 else
               m.Box(parent=s, p0=m.vec3(0.2 * n, 0.4 * n, 0.4 * n), p1=m.vec3(0.3 * n + q, 0.6 * n, 0.6 * n)))
    return mo


def particles(m, torch, st):
    n, s = st["n"], st["s"]
    parts = s.create(m.BasicParticleSystem)
    parts.resizeAll(PARTICLES)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    parts.pos.copy_(torch.rand(3 * PARTICLES, device="cuda", generator=g) * (n + 2) - 1)      # some outside the grid
    parts.flag.copy_(torch.where(torch.rand(PARTICLES, device="cuda", generator=g) < 0.1, 1 << 10, 0).to(torch.int32))
    return parts


def move(m, st, mo):
    n = st["n"]
    return lambda: mo.moveLinear(0.5, 0.0, 1.0, m.vec3(0.3 * n, 0.5 * n, 0.5 * n), m.vec3(0.7 * n, 0.5 * n, 0.5 * n), st["flags"], st["obvel"], True)


def time_state(m, torch, np, st, reps):
    s, n, flags, vel, obvel, phi, phiObs, grad = (st[k] for k in ("s", "n", "flags", "vel", "obvel", "phi", "phiObs", "grad"))
    cells = flags.n
    lib = s.lib
    zero = m.vec3(0, 0, 0)

    def timed(fn, reps=reps, host=False):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6 if host else a.elapsed_time(b) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    scratch = s.create(m.MACGrid)
    copy_us, copy_min = timed(lambda: scratch.copyFrom(vel))
    copy_tbs = 24 * cells / (copy_us * 1e-6) / 1e12
    out = {"dims": [n, n, n], "reps": reps, "copy": {"us": copy_us, "min_us": copy_min, "bytes": 24 * cells, "TBs": copy_tbs}}

    def entry(name, fn, nbytes, **kw):
        us, mn = timed(fn, **kw)
        tbs = nbytes / (us * 1e-6) / 1e12
        out[name] = {"us": us, "min_us": mn, "bytes": int(nbytes), "TBs": tbs, "share_of_measured_copy": tbs / copy_tbs, "share_of_hbm_peak": tbs / HBM_PEAK_TBS}

    band = 12 * (cells - (n - 4) ** 3)
    real, mac = s.create(m.RealGrid), s.create(m.MACGrid)
    entry("setWallBcs (context)", lambda: m.setWallBcs(flags=flags, vel=vel, notiming=True), 28 * cells)
    entry("set_wall_bcs2", lambda: m.set_wall_bcs2(flags, vel, obvel, notiming=True), 4 * cells)
    entry("set_bound_MAC2_w1", lambda: vel.set_bound_MAC2(zero, 1), band)
    entry("setBoundMAC_w1", lambda: vel.setBoundMAC(zero, 1), band)
    entry("setBoundMAC_w1_normalOnly", lambda: vel.setBoundMAC(zero, 1, True), band)
    entry("mark_surface", lambda: flags.mark_surface(), 4 * cells)
    work = s.create(m.FlagGrid)

    def clear():
        work.copyFrom(flags)
        work.clear_obstacle()
    base_us, _ = timed(lambda: work.copyFrom(flags))
    entry("clear_obstacle (with the 8 n copy that restores its input: %.1f us)" % base_us, clear, 12 * cells)

    def clamp(g, src):
        g.copyFrom(src)
        g.clamp_norm(1e-3)
    entry("clamp_norm_real (with the 8 n copy that restores its input)", lambda: clamp(real, phi), 16 * cells)
    entry("clamp_norm_mac (with the 24 n copy that restores its input)", lambda: clamp(mac, vel), 48 * cells)
    entry("resetPhiInObs", lambda: m.resetPhiInObs(flags, phi, notiming=True), 8 * cells)
    passes = 3 * (8 + DISTANCE * 4) * cells + (24 + 28) * cells
    entry("extrapolateMACSimple_plain", lambda: m.extrapolateMACSimple(flags, vel, DISTANCE, notiming=True), passes)
    entry("extrapolateMACSimple_phiObs", lambda: m.extrapolateMACSimple(flags, vel, DISTANCE, phiObs, notiming=True), passes + 16 * cells)
    for k in (1, 8):
        entry("moveLinear_%d_shape%s" % (k, "" if k == 1 else "s"), move(m, st, obstacle(m, st, k)), 8 * cells)
    ls = s.create(m.LevelsetGrid)
    entry("obstacle_sign", lambda: lib.call("mf_movingobs_obstacle_sign", flags.n, flags.ptr, ls.ptr, s.stream), 8 * cells)
    entry("gradient", lambda: lib.call("mf_movingobs_gradient", n, n, n, phiObs.ptr, grad.ptr, s.stream), 16 * cells)
    parts = particles(m, torch, st)
    entry("projectOutside_particles (%d particles; host clock: the host draws the reals between the two kernels)" % PARTICLES,
          lambda: parts.projectOutside(grad), 68 * PARTICLES, reps=max(3, reps // 5), host=True)
    m.resetMovingObstacleState()
    return out


# ---- counting launches and copies: children under rocprofv3 ------------------------------------------------------------------------
def child(what, shapes, calls):
    import torch
    import manta as m
    st = scene(m, torch, 64)
    if what == "move":
        fn = move(m, st, obstacle(m, st, shapes))
    else:
        parts = particles(m, torch, st)
        fn = lambda: parts.projectOutside(st["grad"])
    torch.cuda.synchronize()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def traced(what, shapes, calls):
    """(kernel names, copy directions) of one traced child: a Counter each"""
    tmp = tempfile.mkdtemp(prefix="movingobs_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", what, "--shapes", str(shapes), "--calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        kernels, copies = collections.Counter(), collections.Counter()
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                kernels.update(row.get("Kernel_Name", "?").replace("(anonymous namespace)::", "").split("(")[0] for row in csv.DictReader(f))
        for path in glob.glob(os.path.join(tmp, "**", "*memory_copy_trace.csv"), recursive=True):
            with open(path) as f:
                copies.update(row.get("Direction", "?") for row in csv.DictReader(f))
        return kernels, copies
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def count(calls=10):
    """what one call launches and copies: the trace of 2K calls minus the trace of K calls, over K, by kernel name and by copy direction"""
    out = {"method": "children under rocprofv3 --kernel-trace --memory-copy-trace at 64^3; (trace of %d calls - trace of %d calls) / %d" % (2 * calls, calls, calls)}
    for name, what, shapes in (("moveLinear_1_shape", "move", 1), ("moveLinear_8_shapes", "move", 8), ("projectOutside_particles", "project", 0)):
        k1, c1 = traced(what, shapes, calls)
        k2, c2 = traced(what, shapes, 2 * calls)
        per = lambda a, b: {k: (b[k] - a[k]) / calls for k in sorted(set(a) | set(b)) if b[k] != a[k]}
        row = {"kernels_per_call": per(k1, k2), "copies_per_call": per(c1, c2)}
        row["kernel_launches_per_call"] = sum(row["kernels_per_call"].values())
        # a copy out of the device is a copy-engine transfer or, for a few bytes into pinned host memory, the runtime's own copy kernel
        row["read_backs_per_call"] = (sum(v for k, v in row["copies_per_call"].items() if "DEVICE_TO_HOST" in k.upper())
                                      + sum(v for k, v in row["kernels_per_call"].items() if k.startswith("__amd_rocclr_copy")))
        out[name] = row
    out["claims_hold"] = bool(out["moveLinear_1_shape"]["kernel_launches_per_call"] == out["moveLinear_8_shapes"]["kernel_launches_per_call"] == 2.0
                              and out["projectOutside_particles"]["read_backs_per_call"] == 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="128:256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--count", action="store_true", help="also count launches and read-backs (children under rocprofv3, run first)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--shapes", type=int, default=1)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.shapes, args.calls)
    counted = count() if args.count else None        # before this process opens the GPU
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("movingobs_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_TBs": HBM_PEAK_TBS, "bytes_counted": BYTES, "states": {}}
    for n in (int(v) for v in args.sizes.split(":")):
        st = scene(m, torch, n)
        torch.cuda.synchronize()
        out["states"]["%d^3" % n] = time_state(m, torch, np, st, args.reps)
        del st
        torch.cuda.empty_cache()
    if counted is not None:
        out["counted"] = counted
    line = json.dumps(out)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "movingobs_time.json"), "w") as f:
        f.write(line + "\n")
    if counted is not None and not counted["claims_hold"]:
        raise SystemExit("movingobs_time.py: the counted launches / read-backs are not the claimed ones: %s" % json.dumps(counted))


if __name__ == "__main__":
    main()
