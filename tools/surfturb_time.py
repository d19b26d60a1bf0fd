"""Per-call times of particleSurfaceTurbulence in the dam break of scenes/surfaceTurbulence.py (its loop and its plugin parameters)
at res 32 and res 64.  The first call (initFines and 6 * nb maintenance iterations) is reported on its own; then, after --warmup
further steps, the median / minimum / maximum over --calls calls of: the whole call, its split into cell-list builds, add / delete
(with the rounds of the greedy pass), the normal / regularise / constrain passes, advection and the wave passes, the point counts,
and the call's share of the step.  Every timed window ends in a device synchronise; the host clock is around one call, so launch
and Python overhead are inside.  The split comes from a second run of the same steps with a synchronise around every stage, so it
does not add up exactly to the whole call.

Prints one JSON line and writes it to <out>/surfturb_time.json.  With --stats the same loop runs in a fresh child process under
`rocprofv3 --kernel-trace --stats` (kernel trace only), which leaves its table under <out>/surfturb_stats/.

  python tools/surfturb_time.py [--res 32:64] [--warmup 5] [--calls 10] [--out profiles] [--stats]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = {"coarse_list": "lists", "surface_list": "lists", "init_fines": "initFines", "advect": "advect", "add": "add_delete", "delete": "add_delete",
          "compress_and_insert": "add_delete", "normals": "normals", "regularize": "regularize", "constrain": "constrain", "waves": "waves",
          "save_prev": "output", "displaced": "output"}


def _stats(a):
    import numpy as np
    a = np.asarray(a, float)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def scene(m, st, res):
    """scenes/surfaceTurbulence.py, setup 0 (breaking dam); -> (solver, step function, surface points)"""
    gs = m.vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    s.timestep = 0.8
    flags, phi, vel, velOld, pressure, tmpVec3 = (s.create(t) for t in (m.FlagGrid, m.LevelsetGrid, m.MACGrid, m.MACGrid, m.RealGrid, m.VecGrid))
    spd, pp, sp = (s.create(m.BasicParticleSystem) for _ in range(3))
    pVel, pPrev = pp.create(m.PdataVec3), pp.create(m.PdataVec3)
    nrm = sp.create(m.PdataVec3)
    H, DtH, src, amp, seed = (sp.create(m.PdataReal) for _ in range(5))
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    flags.initDomain(boundaryWidth=1)
    phi = s.create(m.Box, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(0.4, 0.4, 1)).computeLevelset()
    flags.updateFromLevelset(phi)
    m.sampleLevelsetWithParticles(phi=phi, flags=flags, parts=pp, discretization=2, randomness=0.35)
    box = {"phi": phi}

    def fluid():
        phi = box["phi"]
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
        m.mapPartsToMAC(vel=vel, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=tmpVec3)
        m.extrapolateMACFromWeight(vel=vel, distance=2, weight=tmpVec3)
        m.markFluidCells(parts=pp, flags=flags)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phi, 1.0)
        m.resetOutflow(flags=flags, parts=pp, index=gpi, indexSys=pindex)
        m.extrapolateLsSimple(phi=phi, distance=4, inside=True)
        m.addGravity(flags=flags, vel=vel, gravity=(0, -0.001, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure, phi=phi)
        m.setWallBcs(flags=flags, vel=vel)
        pVel.setSource(vel, isMAC=True)
        m.adjustNumber(parts=pp, vel=vel, flags=flags, minParticles=8, maxParticles=16, phi=phi, radiusFactor=1.0)
        m.extrapolateMACSimple(flags=flags, vel=vel)
        m.flipVelocityUpdate(vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.97)

    def plugin():
        st.particleSurfaceTurbulence(flags=flags, coarseParts=pp, coarsePartsPrevPos=pPrev, surfPoints=sp, surfaceNormals=nrm, surfaceWaveH=H,
                                     surfaceWaveDtH=DtH, surfacePointsDisplaced=spd, surfaceWaveSource=src, surfaceWaveSeed=seed,
                                     surfaceWaveSeedAmplitude=amp, res=res, nbSurfaceMaintenanceIterations=6, surfaceDensity=12, outerRadius=1.0,
                                     dt=0.005, waveSpeed=32, waveDamping=0.05, waveSeedFrequency=4.0, waveMaxAmplitude=0.5,
                                     waveMaxSeedingAmplitude=0.5, waveMaxFrequency=128.0, waveSeedingCurvatureThresholdRegionCenter=0.025,
                                     waveSeedingCurvatureThresholdRegionRadius=0.01, waveSeedStepSizeRatioOfMax=0.05)
    return s, fluid, plugin, pp, sp


def run(res, warmup, calls, split):
    import torch
    import manta as m
    from mantaflow_amd import surfturb as st
    st.resetSurfaceTurbulenceState()
    s, fluid, plugin, pp, sp = scene(m, st, res)
    acc = {}
    if split:       # a synchronise and a clock around every stage
        for name, group in STAGES.items():
            fn = getattr(st._Run, name)

            def timed(self, *a, _fn=fn, _group=group, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = _fn(self, *a, **kw)
                torch.cuda.synchronize()
                acc[_group] = acc.get(_group, 0.0) + time.perf_counter() - t0
                return r
            setattr(st._Run, name, timed)
    rows, first = [], None
    for step in range(1 + warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fluid()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        acc.clear()
        plugin()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        s.step()
        info = st.lastSurfaceTurbulenceStats()
        row = {"call_ms": 1e3 * (t2 - t1), "step_ms": 1e3 * (t2 - t0), "coarse": pp.np, "surface": sp.np,
               "rounds": sum(i["rounds"] for i in info["iterations"]), "added": sum(i["added"] for i in info["iterations"]),
               "kills": sum(sum(i["kills"]) for i in info["iterations"]), "split_ms": {k: 1e3 * v for k, v in acc.items()}}
        if step == 0:
            first = row
        elif step > warmup:
            rows.append(row)
    out = {"res": res, "first_call": first, "call_ms": _stats([r["call_ms"] for r in rows]), "step_ms": _stats([r["step_ms"] for r in rows]),
           "share_of_step": _stats([r["call_ms"] / r["step_ms"] for r in rows]), "coarse": rows[-1]["coarse"], "surface": rows[-1]["surface"],
           "rounds_per_call": _stats([r["rounds"] for r in rows]), "added_per_call": _stats([r["added"] for r in rows]),
           "kills_per_call": _stats([r["kills"] for r in rows])}
    if split:
        out["split_ms"] = {k: _stats([r["split_ms"].get(k, 0.0) for r in rows]) for k in sorted(set(STAGES.values()))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="32:64")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sizes = [int(x) for x in a.res.split(":")]
    if a.child:
        for res in sizes:
            run(res, a.warmup, a.calls, False)
        return
    if a.stats:
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(a.out, "surfturb_stats"), "--", sys.executable,
                               os.path.abspath(__file__), "--child", "--res", a.res, "--warmup", str(a.warmup), "--calls", str(a.calls)])
        return
    result = {"warmup": a.warmup, "calls": a.calls, "runs": []}
    for res in sizes:
        whole = run(res, a.warmup, a.calls, False)
        whole["split_ms"] = subprocess_split(res, a)
        result["runs"].append(whole)
    line = json.dumps(result)
    print(line)
    with open(os.path.join(a.out, "surfturb_time.json"), "w") as f:
        f.write(line + "\n")


def subprocess_split(res, a):
    """the split needs the stages wrapped and the process-wide state fresh: a child of its own"""
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import surfturb_time as t; "
            "print('SPLIT ' + json.dumps(t.run(%d, %d, %d, True)['split_ms']))" % (ROOT, os.path.join(ROOT, "tools"), res, a.warmup, a.calls))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("SPLIT ")][-1][6:])


if __name__ == "__main__":
    main()
