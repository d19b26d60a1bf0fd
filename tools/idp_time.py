"""Times of implicit density projection on the GPU: the 3-D scene loop of scenes/idp_apic02_3d.py (a breaking dam, APIC) stepped
with the position solver on beside the same loop with it off, the two alternated step by step in one process, at 64^3 and 128^3.
Per size: whole-step time of both loops, the per-call times of the five plugins and of the position solve's solvePressureSystem,
and the stats of the last mapMassToGrid.  Within the same run the particle->grid share of mapMassToGrid (the weights-only ordered
transfer) is timed against mapPartsToGrid on the same particles, alternated.  Every timed window ends in a device synchronise; the
first --warmup steps of each loop are not timed.  Prints one JSON line.

  python tools/idp_time.py [--warmup N] [--steps N] [--sizes 64:128] [--only-idp]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manta as m  # noqa: E402
from mantaflow_amd import plugins  # noqa: E402
from mantaflow_amd.core import _ptr  # noqa: E402

CALLS = ("copyFlagsToFlags", "mapMassToGrid", "solvePressureSystem", "computeDeltaX", "mapMACToPartPositions")


class Dam(object):
    """scenes/idp_apic02_3d.py at `res`^3 with its shipped settings"""

    def __init__(self, res, position_solver):
        self.on = position_solver
        gs = m.vec3(res, res, res)
        s = self.s = m.Solver(name="main", gridSize=gs, dim=3)
        self.flags, self.vel, self.pressure, self.tmpVec3 = s.create(m.FlagGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.VecGrid)
        self.pp = s.create(m.BasicParticleSystem)
        self.pVel = self.pp.create(m.PdataVec3)
        self.phiObs, self.apic_mass = s.create(m.LevelsetGrid), s.create(m.MACGrid)
        self.cp = [self.pp.create(m.PdataVec3) for _ in range(3)]
        self.density, self.Lambda, self.deltaX, self.flagsPos = s.create(m.RealGrid), s.create(m.RealGrid), s.create(m.MACGrid), s.create(m.FlagGrid)
        self.pMass = self.pp.create(m.PdataReal)
        self.mass = 1.0 / 8
        s.timestep, s.frameLength, s.timestepMin, s.timestepMax, s.cfl = 1, 10000000.0, 0.01, 1.0, 5.0
        self.flags.initDomain(boundaryWidth=1)
        self.flags.updateFromLevelset(m.Box(parent=s, p0=gs * m.vec3(0, 0, 0.25), p1=gs * m.vec3(0.5, 0.35, 0.75)).computeLevelset())
        m.sampleFlagsWithParticles(flags=self.flags, parts=self.pp, discretization=2, randomness=0.5)
        m.copyFlagsToFlags(self.flags, self.flagsPos)
        self.flags.initDomain(boundaryWidth=1, phiWalls=self.phiObs)
        self.calls = {k: [] for k in CALLS}
        self.stats, self.cg = {}, []

    def _timed(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        self.calls[name].append((time.perf_counter() - t0) * 1e3)

    def step(self):
        s, flags, vel, pp, pVel, fp = self.s, self.flags, self.vel, self.pp, self.pVel, self.flagsPos
        cpx, cpy, cpz = self.cp
        s.adaptTimestep(vel.getMax())
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=2, deleteInObstacle=False, stopInObstacle=False)
        if self.on:
            self._timed("copyFlagsToFlags", lambda: m.copyFlagsToFlags(flags, fp))
            self._timed("mapMassToGrid", lambda: m.mapMassToGrid(flags=fp, density=self.density, parts=pp, source=self.pMass, deltaX=self.deltaX,
                                                                 phiObs=self.phiObs, dt=s.timestep, particleMass=self.mass, noDensityClamping=False))
            self.stats = dict(plugins.mapMassToGridStats)
            self._timed("solvePressureSystem", lambda: m.solvePressureSystem(rhs=self.density, vel=vel, pressure=self.Lambda, flags=fp, cgAccuracy=1e-3))
            self.cg.append(int(m.lastCgStats()["iterations"]))
            self._timed("computeDeltaX", lambda: m.computeDeltaX(deltaX=self.deltaX, Lambda=self.Lambda, flags=fp))
            self._timed("mapMACToPartPositions", lambda: m.mapMACToPartPositions(flags=fp, deltaX=self.deltaX, parts=pp, dt=s.timestep))
        m.apicMapPartsToMAC(flags=flags, vel=vel, parts=pp, partVel=pVel, cpx=cpx, cpy=cpy, cpz=cpz, mass=self.apic_mass)
        m.extrapolateMACFromWeight(vel=vel, distance=2, weight=self.tmpVec3)
        m.markFluidCells(parts=pp, flags=flags)
        m.addGravityNoScale(flags=flags, vel=vel, gravity=(0, -0.01, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=self.pressure, cgAccuracy=1e-3)
        m.setWallBcs(flags=flags, vel=vel)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=5)
        m.apicMapMACGridToParts(partVel=pVel, cpx=cpx, cpy=cpy, cpz=cpz, parts=pp, vel=vel, flags=flags)
        s.step()


def spread(ts):
    ts = np.asarray(ts, np.float64)
    return {"median": float(np.median(ts)), "min": float(ts.min()), "max": float(ts.max())}


def p2g_share(d, reps):
    """the weights-only ordered transfer of mapMassToGrid against mapPartsToGrid on the loop's particles, alternated"""
    s, pp = d.s, d.pp
    target = s.create(m.RealGrid)
    ts = {"idp_weights": [], "mapPartsToGrid": []}

    def weights():
        s.lib.call("mf_idp_map_weights", d.flags.sx, d.flags.sy, d.flags.sz, target.ptr, pp.np, pp.cap, _ptr(pp.pos), _ptr(pp.flag), d.pMass.ptr, s.stream)

    for r in range(reps + 2):
        for k, fn in (("idp_weights", weights), ("mapPartsToGrid", lambda: m.mapPartsToGrid(flags=d.flags, target=target, parts=pp, source=d.pMass))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in ts.items()}


def run(res, warmup, steps, only_idp):
    loops = {"position_solver_on": Dam(res, True)}
    if not only_idp:
        loops["position_solver_off"] = Dam(res, False)
    times = {k: [] for k in loops}
    for t in range(warmup + steps):
        for k, d in loops.items():        # alternated: both loops see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.step()
            torch.cuda.synchronize()
            if t >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    on = loops["position_solver_on"]
    out = {"res": res, "warmup_steps": warmup, "timed_steps": steps, "particles": on.pp.pySize(),
           "step_ms": {k: spread(v) for k, v in times.items()},
           "call_ms": {k: spread(on.calls[k][warmup:]) for k in CALLS},
           "position_solve_cg_iterations": on.cg[warmup:], "mapMassToGridStats": on.stats}
    if not only_idp:
        out["p2g_ms"] = p2g_share(on, 10)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", default="64:128")
    ap.add_argument("--only-idp", action="store_true", help="the loop with the position solver alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("idp_time.py needs a GPU")
    out = {"gpu": torch.cuda.get_device_name(0), "sizes": []}
    for spec in args.sizes.split(":"):
        out["sizes"].append(run(int(spec), args.warmup, args.steps, args.only_idp))
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
