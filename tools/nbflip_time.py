"""Times of narrow-band FLIP on the GPU: a dam break stepped with the narrow-band loop (band 3: adjustNumber(narrowBand=3),
combineGridVel(phi, narrowBand=2)) beside the same loop as full FLIP (no band), the two alternated step by step in one process,
at 128^3 and at benchmark_dam.py's 379x356x124.  Per size: whole-step time and particle count of both loops, and the per-call time
of adjustNumber (with its rounds, kills, inserts) and combineGridVel in the narrow-band loop.  Every timed window ends in a device
synchronise; the first --warmup steps of each loop (resampling reaches its steady state) are not timed.  Prints one JSON line.

  python tools/nbflip_time.py [--warmup N] [--steps N] [--sizes 128,128,128:379,356,124] [--only-band]
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

BAND = 3


class Dam(object):
    """the narrow-band dam break of the reference's narrow-band regression scene on a box of `dims` cells; band <= 0: full FLIP"""

    def __init__(self, dims, band):
        self.band = band
        gs = m.vec3(*dims)
        s = self.s = m.Solver(name="dam", gridSize=gs, dim=3)
        s.timestep = 0.9
        self.flags = s.create(m.FlagGrid)
        self.phiParts, self.phi, self.pressure = s.create(m.LevelsetGrid), s.create(m.LevelsetGrid), s.create(m.RealGrid)
        self.vel, self.velOld, self.velParts, self.mapWeights = (s.create(m.MACGrid) for _ in range(4))
        self.pp = s.create(m.BasicParticleSystem)
        self.pVel = self.pp.create(m.PdataVec3)
        self.pindex, self.gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
        self.flags.initDomain(boundaryWidth=0)
        self.phi.initFromFlags(self.flags)
        self.phi.join(s.create(m.Box, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(1.0, 0.15, 1.0)).computeLevelset())
        self.phi.join(s.create(m.Box, p0=gs * m.vec3(0, 0.15, 0), p1=gs * m.vec3(0.4, 0.5, 0.8)).computeLevelset())
        self.flags.updateFromLevelset(self.phi)
        m.sampleLevelsetWithParticles(phi=self.phi, flags=self.flags, parts=self.pp, discretization=2, randomness=0.4)
        m.mapGridToPartsVec3(source=self.vel, parts=self.pp, target=self.pVel)
        self.calls = {"adjustNumber": [], "combineGridVel": []}
        self.stats = []

    def _timed(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        self.calls[name].append((time.perf_counter() - t0) * 1e3)

    def step(self):
        s, flags, vel, phi, pp, pVel = self.s, self.flags, self.vel, self.phi, self.pp, self.pVel
        band = self.band > 0
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=phi, order=1)
        flags.updateFromLevelset(phi)
        m.advectSemiLagrange(flags=flags, vel=vel, grid=vel, order=2, clampMode=1)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=self.pindex, index=self.gpi)
        m.unionParticleLevelset(pp, self.pindex, flags, self.gpi, self.phiParts, radiusFactor=1)
        phi.addConst(1.)
        phi.join(self.phiParts)
        m.extrapolateLsSimple(phi=phi, distance=BAND + 2, inside=True)
        m.extrapolateLsSimple(phi=phi, distance=3)
        flags.updateFromLevelset(phi)
        m.mapPartsToMAC(vel=self.velParts, flags=flags, velOld=self.velOld, parts=pp, partVel=pVel, weight=self.mapWeights)
        m.extrapolateMACFromWeight(vel=self.velParts, distance=2, weight=self.mapWeights)
        if band:
            self._timed("combineGridVel", lambda: m.combineGridVel(vel=self.velParts, weight=self.mapWeights, combineVel=vel, phi=phi,
                                                                    narrowBand=self.band - 1, thresh=0))
        else:
            self._timed("combineGridVel", lambda: m.combineGridVel(vel=self.velParts, weight=self.mapWeights, combineVel=vel, thresh=0))
        self.velOld.copyFrom(vel)
        m.addGravity(flags=flags, vel=vel, gravity=(0, -0.003, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=self.pressure, phi=phi)
        m.setWallBcs(flags=flags, vel=vel)
        m.extrapolateMACSimple(flags=flags, vel=vel, distance=5)
        m.flipVelocityUpdate(vel=vel, velOld=self.velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.95)
        pVel.setSource(vel, isMAC=True)
        self._timed("adjustNumber", lambda: m.adjustNumber(parts=pp, vel=vel, flags=flags, minParticles=8, maxParticles=16, phi=phi,
                                                          narrowBand=float(self.band) if band else -1.))
        self.stats.append(dict(plugins.adjustNumberStats, particles=pp.pySize()))
        s.step()


def spread(ts):
    ts = np.asarray(ts, np.float64)
    return {"median": float(np.median(ts)), "min": float(ts.min()), "max": float(ts.max())}


def run(dims, warmup, steps, only_band):
    loops = {"narrow_band": Dam(dims, BAND)}
    if not only_band:
        loops["full_flip"] = Dam(dims, -1)
    times = {k: [] for k in loops}
    for t in range(warmup + steps):
        for k, d in loops.items():        # alternated: both loops see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.step()
            torch.cuda.synchronize()
            if t >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"dims": list(dims), "warmup_steps": warmup, "timed_steps": steps}
    for k, d in loops.items():
        last = d.stats[-1]
        out[k] = {"step_ms": spread(times[k]), "particles": last["particles"],
                  "adjustNumber_ms": spread(d.calls["adjustNumber"][warmup:]), "combineGridVel_ms": spread(d.calls["combineGridVel"][warmup:]),
                  "adjustNumber_last": {q: last[q] for q in ("rounds", "kills", "inserted", "compresses")},
                  "cg_iterations": int(plugins.lastCgStats()["iterations"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--sizes", default="128,128,128:379,356,124")
    ap.add_argument("--only-band", action="store_true", help="the narrow-band loop alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nbflip_time.py needs a GPU")
    out = {"gpu": torch.cuda.get_device_name(0), "band": BAND, "sizes": []}
    for spec in args.sizes.split(":"):
        out["sizes"].append(run(tuple(int(v) for v in spec.split(",")), args.warmup, args.steps, args.only_band))
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
