"""Per-call times of the vortex particle family: VortexParticleSystem.advectSelf(RK4) at about 4 k, 16 k and 64 k particles seeded by
VPseedK41 in a sphere (one per cell: probability * dt = 1), and applyToMesh(RK4) of about 4 k particles on a createMesh surface of about
200 k nodes.  Median, minimum and maximum of --calls calls after --warmup; every timed window ends in a device synchronise, and every
call starts from the same positions (restored outside the window).  Per case also: pair evaluations per second (4 stages x targets x
sources per call), the share of the first stage's pairs inside the cutoff (counted on the device with torch, outside the timing), and
the workgroups of a stage's launch (64 targets each) against the 256 compute units.  Prints one JSON line and writes it to
<out>/vortex_time.json.

  python tools/vortex_time.py [--warmup 5] [--calls 10] [--out profiles]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CUS, WG = 256, 64


def _stats(a):
    import numpy as np
    a = np.asarray(a)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def inside_share(torch, tpos, tcap, nT, live, vp):
    """share of the (live target, live source) pairs with 1e-8 <= rlen2 <= 6 sigma^2, positions as they are"""
    sp = vp.pos.view(3, vp.cap)[:, :vp.np].double()
    ok = (vp.flag[:vp.np] & 1024) == 0
    cut = 6.0 * (vp.sigma.data[:vp.np] * vp.sigma.data[:vp.np]).double()
    tp = tpos.view(3, tcap)[:, :nT].double()
    inside = pairs = 0
    for a in range(0, nT, 1024):
        b = min(a + 1024, nT)
        d = tp[:, a:b, None].float() - sp[:, None, :].float()
        r2 = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).double()
        m = (r2 <= cut[None, :]) & (r2 >= 1e-8) & ok[None, :] & live[a:b, None]
        inside += int(m.sum().item())
        pairs += int(live[a:b].sum().item()) * int(ok.sum().item())
    return inside / max(pairs, 1)


def timed(torch, fn, restore, warmup, calls):
    ts = []
    for r in range(warmup + calls):
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return _stats(ts)


def seeded(m, s, centre, radius):
    vp = s.create(m.VortexParticleSystem)
    m.VPseedK41(vp, m.Sphere(parent=s, center=m.vec3(*centre), radius=radius), strength=1.0, sigma0=0.2, sigma1=1.0, probability=1.0, N=3.0)
    return vp


def report(torch, out, ms, nT, nS, share):
    out.update(targets=nT, sources=nS, call_ms=ms, pairs_per_call=4 * nT * nS, share_of_pairs_inside_cutoff=round(share, 6),
               pair_evaluations_per_s=4 * nT * nS / (ms["median"] * 1e-3), workgroups_per_stage=(nT + WG - 1) // WG,
               workgroups_per_cu=round(((nT + WG - 1) // WG) / CUS, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vortex_time.py needs a GPU")
    import manta as m
    res = {"gpu": torch.cuda.get_device_name(0), "warmup_calls": args.warmup, "timed_calls": args.calls, "mode": "RK4", "tile_skipping": "not built",
           "advectSelf": {}, "applyToMesh": {}}
    for label, radius in (("4k", 9.85), ("16k", 15.63), ("64k", 24.81)):
        m.resetVortexSeedStream()
        s = m.Solver(name="v", gridSize=m.vec3(64, 64, 64), dim=3)
        s.timestep = 1.0
        vp = seeded(m, s, (32, 32, 32), radius)
        saved = vp.pos.clone()
        live = (vp.flag[:vp.np] & 1024) == 0
        share = inside_share(torch, vp.pos, vp.cap, vp.np, live, vp)
        ms = timed(torch, lambda: vp.advectSelf(scale=1.0, integrationMode=m.IntRK4), lambda: vp.pos.copy_(saved), args.warmup, args.calls)
        res["advectSelf"][label] = report(torch, {}, ms, vp.np, vp.np, share)
    # a sphere's surface of about 200 k nodes, and about 4 k particles around a point of it
    n = 220
    m.resetVortexSeedStream()
    s = m.Solver(name="w", gridSize=m.vec3(n, n, n), dim=3)
    s.timestep = 1.0
    phi = m.Sphere(parent=s, center=m.vec3(n / 2, n / 2, n / 2), radius=0.45 * n).computeLevelset()
    mesh = s.create(m.Mesh)
    phi.createMesh(mesh)
    vp = seeded(m, s, (n / 2 + 0.45 * n, n / 2, n / 2), 9.85)
    saved = mesh.pos.clone()
    live = (mesh.nflag[:mesh.nn] & 1) == 0
    share = inside_share(torch, mesh.pos, mesh.ncap, mesh.nn, live, vp)
    ms = timed(torch, lambda: vp.applyToMesh(mesh, scale=1.0, integrationMode=m.IntRK4), lambda: mesh.pos.copy_(saved), args.warmup, args.calls)
    res["applyToMesh"]["4k_on_200k"] = report(torch, {"grid": [n, n, n]}, ms, mesh.nn, vp.np, share)
    m.resetVortexSeedStream()
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "vortex_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
