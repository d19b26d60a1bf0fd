"""Times of the multigrid preconditioner on 2-D solvers (PcMGStatic / PcMGDynamic behind mantaflow_amd.multigrid2d) against the only
2-D route there was before it, preconditioner=PcMIC -- which on a 2-D solver is plain CG with the x4 iteration cap
(conjugategrad.cpp:315-321, pressure.cpp:410; that route's code is not touched by the 2-D hierarchy, so this tree's library is the
parent's for it) -- on one GPU, alternating in one process so clocks and cache state are shared.  Two inputs per size n x n:
  smoke  scenes/plume_2d.py's set-up (initDomain(1), fillGrid, open top and bottom), a smooth velocity after setWallBcs, cgAccuracy 1e-3
  liq    util.make_flags(seed 1, obstacle blobs, empty top third), smooth velocity, cgAccuracy 1e-5 with the L2 norm
Per input and size: medians of --reps solves after --warmup, with min - max, of solvePressureSystem with PcMIC, PcMGStatic in steady
state (hierarchy kept) and PcMGDynamic (set-up in every solve); CG iterations; the set-up's host / device microseconds (info());
one V-cycle by device events and its launch count (counted from the level table: the grid-wide levels take colours + 2 launches
down and colours + 1 up, the tail one, set_rhs one; the copy of the result is a copy, not a launch).  At --sweep-size, one sweep of
MF_MG_TAIL_VERTS (the hand-over from the grid-wide kernels to the single-workgroup tail) over 0, 2048, 8192, 32768.

At these sizes every level but the first one or two is cache-resident and every pass on them is launch-bound: the figures are
figures of launch counts and host pacing as much as of kernels.

  python tools/mg2d_time.py [--sizes 256,1024,2048] [--reps 10] [--warmup 5] [--sweep-size 1024] [--out-dir profiles]
Writes <out-dir>/mg2d_time.json.  Every size is a child process under its own time limit; after one that fails nothing more is started."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWEEP = (0, 2048, 8192, 32768)


def inputs(kind, n):
    import numpy as np
    import util
    if kind == "smoke":
        flags = util.make_flags(n, n, 1, seed=1, obstacles=False, bw=1)      # initDomain(boundaryWidth=1) + fillGrid
        for rows in (slice(0, 2), slice(n - 2, n)):                          # setOpenBound(flags, 1, 'yY', FlagOutflow | FlagEmpty)
            band = flags[:, rows, 2:n - 2]
            band[...] = util.EMPTY | util.OUTFLOW
        return flags, util.smooth_vel(n, n, 1, 1), dict(cgAccuracy=1e-3)
    flags = util.make_flags(n, n, 1, seed=1, obstacles=True, empty_top=True)
    return flags, util.smooth_vel(n, n, 1, 1), dict(cgAccuracy=1e-5, useL2Norm=True)


class Scene(object):
    """a 2-D solver holding the system of one input"""

    def __init__(self, n, flags, vel, kw):
        import cases
        from mantaflow_amd import core, plugins
        self.plugins, self.kw = plugins, kw
        self.s = cases._mk_solver((n, n, 1))
        self.fl, self.v, self.p, self.rhs = core.FlagGrid(self.s), core.MACGrid(self.s), core.Grid(self.s), core.Grid(self.s)
        cases.soa_to_grid(self.fl, flags)
        cases.soa_to_grid(self.v, vel)
        plugins.setWallBcs(self.fl, self.v)
        plugins.computePressureRhs(self.rhs, self.v, self.p, self.fl, **kw)
        self.rhs0 = self.rhs.data.clone()

    def solve(self, pc):
        import torch
        self.rhs.data.copy_(self.rhs0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.plugins.solvePressureSystem(self.rhs, self.v, self.p, self.fl, preconditioner=pc, **self.kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, self.plugins.lastCgStats()["iterations"]


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4), n=len(xs))


def vcycle(scene, reps):
    """one V-cycle on the solver's kept hierarchy by device events -> stats, info()"""
    import ctypes
    import torch
    mg = scene.s._mg
    dst, src = torch.zeros_like(scene.rhs0), scene.rhs0
    call = lambda: scene.s.lib.call("mf_mg2d_vcycle", mg.handle, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), scene.s.stream)
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return stats(out), mg.info()


def launches(info):
    first = info["tail_first_level"]
    per_level = [(2 if l == 0 else 4) for l in range(first)]
    return 1 + sum(c + 2 for c in per_level) + 1 + sum(c + 1 for c in per_level)


def step_size(args, n):
    import torch
    from mantaflow_amd import multigrid2d
    from mantaflow_amd.plugins import PcMGDynamic, PcMGStatic, PcMIC
    assert torch.cuda.is_available(), "mg2d_time.py needs a GPU"
    multigrid2d.setMultigrid2D()
    res = dict(size=n, device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, inputs={})
    for kind in ("smoke", "liq"):
        flags, vel, kw = inputs(kind, n)
        sc = Scene(n, flags, vel, kw)
        routes = (("cg_pcmic", PcMIC), ("mg_static", PcMGStatic), ("mg_dynamic", PcMGDynamic))
        t, it = {k: [] for k, _ in routes}, {}
        for i in range(args.warmup + args.reps):      # alternating: one solve of each route per round
            for name, pc in routes:
                if name == "mg_dynamic":
                    kept = sc.s._mg                   # Dynamic releases the solver's hierarchy: park Static's for its next turn
                    sc.s._mg = None
                ms, it[name] = sc.solve(pc)
                if name == "mg_dynamic":
                    sc.s._mg = kept
                if name == "mg_static":
                    p_static = sc.p.data.clone()
                elif name == "mg_dynamic":
                    assert torch.equal(sc.p.data, p_static), "Static (steady state, same flags) and Dynamic disagree"
                if i >= args.warmup:
                    t[name].append(ms)
        info = sc.s._mg.info()
        assert info["setups"] == 1
        vc, info = vcycle(sc, max(args.reps, 20))
        r = {k: dict(stats(v), iterations=it[k]) for k, v in t.items()}
        r["setup"] = dict(host_selection_us=info["setup_host_us"], device_and_copies_us=info["setup_device_us"])
        r["vcycle"] = dict(vc, launches=launches(info), coarse_cg_iterations=info["coarse_cg_iterations"], tail_first_level=info["tail_first_level"])
        r["levels"] = dict(sizes=info["sizes"], active=info["active"])
        for k in ("mg_static", "mg_dynamic"):
            r["ratio_cg_pcmic_over_" + k] = dict(median=round(r["cg_pcmic"]["median_ms"] / r[k]["median_ms"], 3),
                                                 low=round(r["cg_pcmic"]["min_ms"] / r[k]["max_ms"], 3), high=round(r["cg_pcmic"]["max_ms"] / r[k]["min_ms"], 3))
        sc.plugins.releaseMG(sc.s)
        if n == args.sweep_size:
            sweep = {}
            for verts in SWEEP:
                os.environ["MF_MG_TAIL_VERTS"] = str(verts)      # read at every create
                try:
                    for _ in range(args.warmup):
                        sc.solve(PcMGStatic)
                    assert torch.equal(sc.p.data, p_static), "the hand-over changes the result"
                    ts = [sc.solve(PcMGStatic)[0] for _ in range(args.reps)]
                    v, inf = vcycle(sc, max(args.reps, 20))
                    sweep[str(verts)] = dict(solve=stats(ts), vcycle=v, launches=launches(inf), tail_first_level=inf["tail_first_level"])
                    sc.plugins.releaseMG(sc.s)
                finally:
                    del os.environ["MF_MG_TAIL_VERTS"]
            r["tail_verts_sweep"] = sweep
        res["inputs"][kind] = r
        print(n, kind, json.dumps(r), flush=True)
        del sc
    with open(os.path.join(args.out_dir, "_mg2d_time_%d.json" % n), "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep-size", type=int, default=1024)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", type=int, help="(internal) time one size in this process")
    args = ap.parse_args()
    args.out_dir = os.path.abspath(args.out_dir)
    os.makedirs(args.out_dir, exist_ok=True)
    if args.step:
        return step_size(args, args.step)
    sizes = [int(s) for s in args.sizes.split(",")]
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup), "--sweep-size", str(args.sweep_size),
          "--out-dir", args.out_dir]
    out = dict(sizes={})
    for n in sizes:
        rc = subprocess.call(["timeout", "-k", "10", "300"] + me + ["--step", str(n)])
        if rc != 0:
            sys.exit("mg2d_time.py: size %d ended with status %d; nothing more is run" % (n, rc))
        part = os.path.join(args.out_dir, "_mg2d_time_%d.json" % n)
        r = json.load(open(part))
        os.remove(part)
        out.update(device=r["device"], reps=r["reps"], warmup=r["warmup"])
        out["sizes"][str(n)] = r["inputs"]
    with open(os.path.join(args.out_dir, "mg2d_time.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("mg2d_time.py: wrote", os.path.join(args.out_dir, "mg2d_time.json"))


if __name__ == "__main__":
    main()
