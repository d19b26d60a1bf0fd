"""Times of the fill-fraction obstacle plugins on the GPU: fraction-mode setWallBcs, updateFractions and setObstacleFlags at 256^3
(a sphere of radius 0.2 * res inside walls), and one karman-style 3-D step at 256x128x128 (advect, extrapolateMACSimple(intoObs),
setWallBcs(fractions), setInflowBcs, solvePressure(fractions)).  Prints one JSON line.

  python tools/obstacle_time.py [--reps N]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manta as m  # noqa: E402
from mantaflow_amd import plugins  # noqa: E402


def scene(dims, center, radius):
    sx, sy, sz = dims
    s = m.Solver(name="t", gridSize=m.vec3(*dims), dim=3)
    flags, phiObs, fr, vel = s.create(m.FlagGrid), s.create(m.LevelsetGrid), s.create(m.MACGrid), s.create(m.MACGrid)
    flags.initDomain(boundaryWidth=0, inflow="xX")
    k, j, i = torch.meshgrid(*(torch.arange(n, device="cuda", dtype=torch.float32) for n in (sz, sy, sx)), indexing="ij")
    d = torch.sqrt((i + 0.5 - center[0]) ** 2 + (j + 0.5 - center[1]) ** 2 + (k + 0.5 - center[2]) ** 2) - radius
    d = torch.minimum(d, torch.minimum(j - 0.5, sy - 1.5 - j))
    d = torch.minimum(d, torch.minimum(k - 0.5, sz - 1.5 - k))
    phiObs.data.copy_(d.reshape(-1))
    del i, j, k, d
    m.updateFractions(flags=flags, phiObs=phiObs, fractions=fr)
    m.setObstacleFlags(flags=flags, phiObs=phiObs, fractions=fr)
    flags.fillGrid()
    vel.setConst(m.vec3(0.9, 0, 0))
    return s, flags, phiObs, fr, vel


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    res = 256
    s, flags, phiObs, fr, vel = scene((res, res, res), (0.5 * res, 0.5 * res, 0.5 * res), 0.2 * res)
    flags2 = s.create(m.FlagGrid)
    flags2.copyFrom(flags)
    out = {"gpu": torch.cuda.get_device_name(0), "res": res}
    out["setWallBcs_frac_us"], out["setWallBcs_frac_min_us"] = timed(
        lambda: m.setWallBcs(flags=flags, vel=vel, fractions=fr, phiObs=phiObs, notiming=True), args.reps)
    out["updateFractions_us"], out["updateFractions_min_us"] = timed(
        lambda: m.updateFractions(flags=flags, phiObs=phiObs, fractions=fr, notiming=True), args.reps)
    out["setObstacleFlags_us"], out["setObstacleFlags_min_us"] = timed(
        lambda: m.setObstacleFlags(flags=flags2, phiObs=phiObs, fractions=fr, notiming=True), args.reps)
    out["setWallBcs_plain_us"], _ = timed(lambda: m.setWallBcs(flags=flags, vel=vel, notiming=True), args.reps)
    del s, flags, flags2, phiObs, fr, vel
    torch.cuda.empty_cache()

    dims = (2 * 128, 128, 128)
    s, flags, phiObs, fr, vel = scene(dims, (0.25 * dims[0], 0.5 * dims[1], 0.5 * dims[2]), 0.2 * dims[1])
    pressure = s.create(m.RealGrid)
    inflow = m.vec3(0.9, 0, 0)
    iters = []

    def step():
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=2, intoObs=True)
        m.setWallBcs(flags=flags, vel=vel, fractions=fr, phiObs=phiObs)
        m.setInflowBcs(vel=vel, dir="xX", value=inflow)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, fractions=fr, cgAccuracy=1e-4, cgMaxIterFac=5.0)
        iters.append(plugins.lastCgStats()["iterations"])

    out["karman3d_dims"] = list(dims)
    out["karman3d_step_ms"], out["karman3d_step_min_ms"] = (v / 1e3 for v in timed(step, max(3, args.reps // 10)))
    out["karman3d_cg_iterations"] = iters[-1]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
