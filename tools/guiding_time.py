"""Times of PD_fluid_guiding on the guided plume of scenes/guiding_3d02_high.py: the fine solver at the scene's 80x160x80 and at
128x256x128, the target velocity from an in-process coarse plume (half the resolution, scenes/guiding_3d01_low.py's loop) through
interpolateMACGrid -- no files are read.  Per size, after --warmup guided steps, medians over --calls:

  * the plugin's time per call and its primal-dual iterations, beside the same loop composed -- inside this tool only -- from the
    per-operation grid methods (copyFrom / multConst / add / mult / sub / addScaled / getMaxAbs) around the same blur and the same
    solvePressure: the yardstick for what the three fused kernels buy.  The two are alternated from the same starting state and
    must end in the same velocity, bit for bit;
  * one iteration's parts alone: the inner solve, the two blurs, the fused element-wise kernels (and their composed counterpart);
  * a 1-D blur pass as a fraction of the HBM peak (8 TB/s) on 24 B per cell.

Every timed window ends in a device synchronise.  Prints one JSON line and writes it to <out>/guiding_time.json; with --stats, a child
process first runs the smaller size alone under `rocprofv3 --kernel-trace --stats` and its kernel table becomes
<out>/guiding_kernel_stats.csv.

  python tools/guiding_time.py [--warmup 2] [--calls 5] [--sizes 80:128] [--out profiles] [--stats]
"""
import argparse
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

HBM_PEAK = 8.0e12
BETA, W_SCALAR, THETA = 5, 2, 0.3
TAU = 0.58 / W_SCALAR
SIGMA = 2.44 / TAU


def plume(m, res, name):
    """the common part of guiding_3d01_low.py / guiding_3d02_high.py: solver, grids, noise, open yY bounds, source"""
    gs = m.vec3(res, 2 * res, res)
    s = m.Solver(name=name, gridSize=gs, dim=3)
    s.timestep = 0.65
    g = dict(s=s, flags=s.create(m.FlagGrid), vel=s.create(m.MACGrid), density=s.create(m.RealGrid), pressure=s.create(m.RealGrid))
    noise = s.create(m.NoiseField, loadFromFile=True)
    noise.posScale = m.vec3(0)
    noise.clamp = True
    noise.clampNeg = 0
    noise.clampPos = 1
    noise.valScale = 1
    noise.valOffset = 0.75
    noise.timeAnim = 0.2
    g["flags"].initDomain(boundaryWidth=0)
    g["flags"].fillGrid()
    m.setOpenBound(g["flags"], 0, "yY", m.FlagOutflow | m.FlagEmpty)
    g["noise"] = noise
    g["source"] = s.create(m.Cylinder, center=gs * m.vec3(0.5, 0.05, 0.5), radius=res * 0.1, z=gs * m.vec3(0, 0.02, 0))
    return g


def advance(m, g, gravity):
    m.densityInflow(flags=g["flags"], density=g["density"], noise=g["noise"], shape=g["source"], scale=1, sigma=0.5)
    m.advectSemiLagrange(flags=g["flags"], vel=g["vel"], grid=g["density"], order=2)
    m.advectSemiLagrange(flags=g["flags"], vel=g["vel"], grid=g["vel"], order=2)
    m.resetOutflow(flags=g["flags"], real=g["density"])
    m.setWallBcs(flags=g["flags"], vel=g["vel"])
    m.addBuoyancy(density=g["density"], vel=g["vel"], gravity=m.vec3(0, gravity, 0), flags=g["flags"])


def guide(m, hi, velT, vel=None):
    m.PD_fluid_guiding(vel=vel or hi["vel"], velT=velT, flags=hi["flags"], weight=hi["W"], blurRadius=BETA, pressure=hi["pressure"], tau=TAU,
                       sigma=SIGMA, theta=THETA, preconditioner=m.PcMGStatic, zeroPressureFixing=True)


def solve(m, hi, z):
    m.solvePressure(z, hi["pressure"], hi["flags"], 1e-3, None, None, None, None, 1e-04, 1.5, True, m.PcMGStatic, False, False, True, None, 0.)


class Parts(object):
    """the pieces of one iteration on the library's entry points, and the same from grid methods"""

    def __init__(self, m, hi, velT):
        from mantaflow_amd import plugins
        self.m, self.hi, self.s = m, hi, hi["s"]
        s = self.s
        self.lib = s.lib
        self.w_dev = plugins._blur_weights(s.lib, s, BETA)
        mk = lambda: s.create(m.MACGrid)
        self.x, self.y, self.z, self.zn, self.Q, self.velC, self.xv, self.vn, self.s1, self.s2, self.x0, self.r = (mk() for _ in range(12))
        self.invA, self.invA3 = s.create(m.RealGrid), mk()
        self.velC.copyFrom(hi["vel"])
        self.Q.copyFrom(velT)
        self.Q.sub(self.velC)
        self.blur2(self.Q)
        self.Q.multConst(m.vec3(2.0))
        self.Q.addScaled(self.velC, m.vec3(float(-self.f(SIGMA))))
        self.lib.call("mf_guiding_inv_a", self.Q.n, hi["W"].ptr, float(self.f(SIGMA)), self.invA.ptr, s.stream)
        for c in range(3):
            self.lib.call("mf_copy_f32", self.Q.n, ctypes.c_void_p(self.invA3.data[c * self.Q.n:].data_ptr()), self.invA.ptr, s.stream)

    @staticmethod
    def f(v):
        import numpy as np
        return np.float32(v)

    def blur2(self, g):
        fl = self.hi["flags"]
        self.lib.call("mf_guiding_blur", fl.sx, fl.sy, fl.sz, fl.ptr, g.ptr, self.s1.ptr, self.s2.ptr, ctypes.c_void_p(self.w_dev.data_ptr()), BETA, 2,
                      self.s.stream)

    # -- fused --
    def pre(self):
        f = self.f
        self.lib.call("mf_guiding_pre", self.x.n, self.x.ptr, self.y.ptr, self.Q.ptr, self.invA.ptr, self.xv.ptr, self.vn.ptr,
                      float(f(1.0 / float(f(SIGMA)))), float(f(SIGMA)), self.s.stream)

    def mid(self):
        f = self.f
        self.lib.call("mf_guiding_mid", self.x.n, self.x.ptr, self.y.ptr, self.xv.ptr, self.vn.ptr, self.invA.ptr, self.velC.ptr, self.z.ptr,
                      self.zn.ptr, float(f(SIGMA)), float(f(TAU)), self.s.stream)
        self.z, self.zn = self.zn, self.z

    def post(self):
        out = (ctypes.c_float * 2)()
        self.lib.call("mf_guiding_post", self.x.n, self.z.ptr, self.zn.ptr, self.y.ptr, float(self.f(THETA)), out, self.s.stream)
        return out[0], out[1]

    # -- composed from grid methods (fluidguiding.cpp:229-239, 266-271, 323-344 call by call) --
    def c_pre(self):
        m, f, x = self.m, self.f, self.x
        self.x0.copyFrom(x)
        x.multConst(m.vec3(float(f(1.0 / float(f(SIGMA))))))
        x.add(self.y)
        x.multConst(m.vec3(float(f(SIGMA))))
        x.add(self.Q)
        self.vn.copyFrom(x)
        self.vn.mult(self.invA3)

    def c_mid(self):
        m, f, x = self.m, self.f, self.x
        self.vn.multConst(m.vec3(2.0))
        self.vn.mult(self.invA3)
        x.mult(self.invA3)
        x.sub(self.vn)
        x.add(self.velC)
        x.multConst(m.vec3(float(-f(SIGMA))))
        x.addScaled(self.y, m.vec3(float(f(SIGMA))))
        x.add(self.x0)
        self.zn.copyFrom(self.z)                      # z0
        self.z.addScaled(x, m.vec3(float(-f(TAU))))

    def c_post(self):
        m, f = self.m, self.f
        self.y.copyFrom(self.z)
        self.y.sub(self.zn)
        self.y.multConst(m.vec3(float(f(THETA))))
        self.y.add(self.z)
        self.r.copyFrom(self.z)                       # getRNorm
        self.r.sub(self.zn)
        return self.r.getMaxAbs(), self.z.getMaxAbs()


def composed_guiding(m, hi, velT, vel, max_iters=200, eps_rel=1e-3, eps_abs=1e-3):
    """PD_fluid_guiding from grid methods around the same blur and solve; returns the iteration count"""
    import numpy as np
    f = np.float32
    p = Parts(m, dict(hi, vel=vel), velT)
    it = 0
    for it in range(max_iters):
        p.c_pre()
        p.blur2(p.vn)
        p.c_mid()
        solve(m, hi, p.z)
        rnorm, zmax = p.c_post()
        eps = f(np.sqrt(3.0) * float(f(eps_abs)) + float(f(eps_rel) * f(zmax)))
        if (it > 0 and f(rnorm) < eps) or it == max_iters - 1:
            break
    vel.copyFrom(p.z)
    return it


def med(a):
    import numpy as np
    a = np.asarray(a, float)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def time_size(m, torch, res, warmup, calls):
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    lo, hi = plume(m, res // 2, "low"), plume(m, res, "high")
    s = hi["s"]
    hi["W"] = s.create(m.RealGrid)
    hi["W"].setConst(W_SCALAR)
    velT, v_fused, v_comp, start = (s.create(m.MACGrid) for _ in range(4))
    t_fused, t_comp, iters, same = [], [], [], True
    m.releaseBlurPrecomp()
    for step in range(warmup + calls):
        advance(m, lo, -1e-3)
        m.solvePressure(flags=lo["flags"], vel=lo["vel"], pressure=lo["pressure"])
        m.setWallBcs(flags=lo["flags"], vel=lo["vel"])
        lo["s"].step()
        advance(m, hi, -2e-3)
        m.interpolateMACGrid(source=lo["vel"], target=velT)
        velT.multConst(m.vec3(2))
        start.copyFrom(hi["vel"])
        order = ("fused", "composed") if step % 2 == 0 else ("composed", "fused")        # alternated, from the same state
        for which in order:
            if which == "fused":
                v_fused.copyFrom(start)
                tf, _ = timed(lambda: guide(m, hi, velT, v_fused))
                nf = m.lastGuidingStats()
            else:
                v_comp.copyFrom(start)
                tc, nc = timed(lambda: composed_guiding(m, hi, velT, v_comp))
        same = same and nf["iterations"] == nc and bool(torch.equal(v_fused.data, v_comp.data))
        if step >= warmup:
            t_fused.append(tf)
            t_comp.append(tc)
            iters.append(nf["iterations"])
        hi["vel"].copyFrom(v_fused)
        m.setWallBcs(flags=hi["flags"], vel=hi["vel"])
        s.step()
    # one iteration's parts, on the state the last step left (alternated)
    p = Parts(m, hi, velT)
    n = p.x.n
    parts = {k: [] for k in ("solve", "blur2", "fused_elementwise", "composed_elementwise")}
    for r in range(warmup + calls):
        row = {}
        a, _ = timed(p.pre)
        row["blur2"], _ = timed(lambda: p.blur2(p.vn))
        b, _ = timed(p.mid)
        row["solve"], _ = timed(lambda: solve(m, hi, p.z))
        c, _ = timed(p.post)
        row["fused_elementwise"] = a + b + c
        a, _ = timed(p.c_pre)
        p.blur2(p.vn)
        b, _ = timed(p.c_mid)
        solve(m, hi, p.z)
        c, _ = timed(p.c_post)
        row["composed_elementwise"] = a + b + c
        if r >= warmup:
            for k, v in row.items():
                parts[k].append(v)
    out = {"dims": [res, 2 * res, res], "cells": n, "warmup_steps": warmup, "timed_steps": calls, "pd_iterations": iters,
           "fused_equals_composed_bitwise": same, "call_ms": med(t_fused), "composed_call_ms": med(t_comp),
           "composed_over_fused_call": round(med(t_comp)["median"] / med(t_fused)["median"], 3),
           "per_iteration_ms": {k: med(v) for k, v in parts.items()}}
    pass_s = out["per_iteration_ms"]["blur2"]["median"] * 1e-3 / 6                     # two 3-D blurs = six 1-D passes
    out["blur_pass_fraction_of_hbm_peak"] = round(24.0 * n / pass_s / HBM_PEAK, 4)
    out["composed_over_fused_elementwise"] = round(out["per_iteration_ms"]["composed_elementwise"]["median"] /
                                                   out["per_iteration_ms"]["fused_elementwise"]["median"], 3)
    m.releaseMG(s)
    m.releaseBlurPrecomp()
    return out


def kernel_stats(out_dir, size, warmup, calls):
    """the smaller size alone in a child process under rocprofv3; its kernel table is copied to out_dir"""
    tmp = tempfile.mkdtemp(prefix="guiding_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--sizes", str(size), "--warmup", str(warmup), "--calls", str(calls), "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=540)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        shutil.copyfile(found[0], os.path.join(out_dir, "guiding_kernel_stats.csv"))
        return True
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sizes", default="80:128", help="res2 of the fine solver (res2 x 2 res2 x res2), colon-separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the first size (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sizes = [int(v) for v in args.sizes.split(":")]
    stats = kernel_stats(args.out, sizes[0], 1, 2) if args.stats else None       # before this process opens the GPU
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("guiding_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "blurRadius": BETA, "sizes": {}}
    for res in sizes:
        out["sizes"]["%dx%dx%d" % (res, 2 * res, res)] = time_size(m, torch, res, args.warmup, args.calls)
        torch.cuda.empty_cache()
    if stats:
        out["kernel_stats"] = "guiding_kernel_stats.csv"
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        with open(os.path.join(args.out, "guiding_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
