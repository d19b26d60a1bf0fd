"""Times of the multigrid preconditioner (PcMGStatic / PcMGDynamic) against the MIC(0) PCG of the PARENT commit's library, at 256^3 on
the GPU, alternating in one process so clocks and cache state are shared.  Two inputs:
  smoke  bench.py's smoke step up to the solve (closed box, synthetic velocity, MacCormack-advected, setWallBcs), zeroPressureFixing,
         cgAccuracy 1e-3 (the fixing makes the system regular: the reference's multigrid does not converge on the singular one)
  liq    util.make_flags(seed 1, obstacle blobs, empty top third), smooth velocity, cgAccuracy 1e-5 with the L2 norm
Timed per input: solvePressureSystem(PcMIC) through the parent's library, through this tree's library, PcMGStatic in steady state
(hierarchy kept), PcMGDynamic (set-up in every solve), the set-up split into host selection / everything else (mf_mg_info), one
V-cycle (device events), and one V-cycle with the single-workgroup tail reduced to the coarsest-level CG (MF_MG_TAIL_VERTS=0), whose
k_mg_tail<Mg3d> time in the kernel statistics (k_mg_tail in the records of before mg_driver.h) is the ordered coarsest solve alone.

The parent's library is not built here (the tree that runs may not be a git checkout).  Build it once from the parent commit:
  git archive <parent> mantaflow_amd/csrc include | tar -x -C <dir> && make -f <dir>/mantaflow_amd/csrc/Makefile
and pass the resulting libmanta_hip.so as --parent-lib (default: build/parent/libmanta_hip_parent.so).

  python tools/mg_time.py [--grid 256] [--reps 7] [--out-dir profiles] [--parent-lib PATH]
Writes <out-dir>/mg_time.json and, from a rocprofv3 --kernel-trace --stats run of its own (one PcMGStatic solve per input, no
counters), <out-dir>/mg_kernel_stats.csv (+ mg_kernel_stats_cgonly.csv for the MF_MG_TAIL_VERTS=0 run).  Every step is a child
process under its own time limit; after a step that fails nothing more is started."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def inputs(kind, n):
    import numpy as np
    import bench
    import cases
    import util
    dims = (n, n, n)
    if kind == "smoke":
        flags = bench.domain_flags(n, n, n)
        vel = bench.synthetic_velocity(n, n, n)
        dens = bench.synthetic_density(n, n, n)
        vel = cases.run_smoke_step_pkg(dims, 1.0, flags, vel, dens)["vel_adv"]
        return flags, vel, dict(cgAccuracy=1e-3, zeroPressureFixing=True)
    flags = util.make_flags(n, n, n, seed=1, obstacles=True, empty_top=True)
    vel = util.smooth_vel(n, n, n, 1)
    return flags, vel, dict(cgAccuracy=1e-5, useL2Norm=True)


class Scene(object):
    """a solver on the library that is current when it is made, holding the system of one input"""

    def __init__(self, n, flags, vel, kw):
        import cases
        from mantaflow_amd import core, plugins
        self.plugins, self.kw = plugins, kw
        self.s = cases._mk_solver((n, n, n))
        self.fl, self.v, self.p, self.rhs = core.FlagGrid(self.s), core.MACGrid(self.s), core.Grid(self.s), core.Grid(self.s)
        cases.soa_to_grid(self.fl, flags)
        cases.soa_to_grid(self.v, vel)
        plugins.setWallBcs(self.fl, self.v)
        plugins.computePressureRhs(self.rhs, self.v, self.p, self.fl, **kw)
        self.rhs0 = self.rhs.data.clone()

    def solve(self, pc):
        import torch
        self.rhs.data.copy_(self.rhs0)      # zero pressure fixing edits the rhs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.plugins.solvePressureSystem(self.rhs, self.v, self.p, self.fl, preconditioner=pc, **self.kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, self.plugins.lastCgStats()["iterations"]


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4), n=len(xs))


def vcycle_ms(scene, reps):
    import ctypes
    import torch
    mg = scene.s._mg
    dst, src = torch.zeros_like(scene.rhs0), scene.rhs0
    call = lambda: scene.s.lib.call("mf_mg_vcycle", mg.handle, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), scene.s.stream)
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


def step_time(args):
    import torch
    from mantaflow_amd import _lib
    from mantaflow_amd.plugins import PcMGDynamic, PcMGStatic, PcMIC
    assert torch.cuda.is_available(), "mg_time.py needs a GPU"
    n = args.grid
    res = dict(grid=n, device=torch.cuda.get_device_name(0), reps=args.reps, inputs={})
    for kind in ("smoke", "liq"):
        _lib.reset()
        flags, vel, kw = inputs(kind, n)
        ours = Scene(n, flags, vel, kw)
        _lib.use_library(args.parent_lib, "cuda")
        parent = Scene(n, flags, vel, kw)
        assert parent.s.lib.path == args.parent_lib and not parent.s.lib.multigrid
        _lib.reset()
        t = {k: [] for k in ("parent_mic", "mic", "mg_static", "mg_dynamic")}
        it = {}
        # warm-up of every route (the first Static solve builds the hierarchy that the later ones keep)
        parent.solve(PcMIC); ours.solve(PcMIC); ours.solve(PcMGStatic)
        setup = ours.s._mg.info()
        for _ in range(args.reps):
            for name, sc, pc in (("parent_mic", parent, PcMIC), ("mic", ours, PcMIC), ("mg_static", ours, PcMGStatic)):
                ms, it[name] = sc.solve(pc)
                t[name].append(ms)
        p_static = ours.p.data.clone()
        assert ours.s._mg.info()["setups"] == 1
        vc, info = vcycle_ms(ours, max(args.reps, 20))
        for _ in range(max(3, args.reps // 2)):
            ms, it["mg_dynamic"] = ours.solve(PcMGDynamic)
            t["mg_dynamic"].append(ms)
        assert torch.equal(ours.p.data, p_static), "Static (steady state, same flags) and Dynamic disagree"
        os.environ["MF_MG_TAIL_VERTS"] = "0"
        try:
            ours.solve(PcMGStatic)
            vc0, info0 = vcycle_ms(ours, max(args.reps, 20))
            assert torch.equal(ours.p.data, p_static), "the tail split changes the result"
            ours.plugins.releaseMG(ours.s)
        finally:
            del os.environ["MF_MG_TAIL_VERTS"]
        r = {k: dict(stats(v), iterations=it[k]) for k, v in t.items()}
        r["setup"] = dict(host_selection_ms=setup["setup_host_us"] / 1e3, device_and_copies_ms=setup["setup_device_us"] / 1e3)
        r["vcycle"] = dict(vc, coarse_cg_iterations=info["coarse_cg_iterations"], tail_first_level=info["tail_first_level"])
        r["vcycle_tail_cg_only"] = dict(vc0, tail_first_level=info0["tail_first_level"])
        r["levels"] = dict(sizes=info["sizes"], active=info["active"])
        r["speedup_static_vs_parent_mic"] = round(r["parent_mic"]["median_ms"] / r["mg_static"]["median_ms"], 3)
        res["inputs"][kind] = r
        print(kind, json.dumps(r), flush=True)
        del ours, parent
    with open(os.path.join(args.out_dir, "mg_time.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def step_profile(args):
    """what runs under rocprofv3: per input one warm-up and one traced-with-the-rest PcMGStatic solve (the statistics cover both,
    the set-up kernels once)"""
    from mantaflow_amd.plugins import PcMGStatic
    for kind in ("smoke", "liq"):
        flags, vel, kw = inputs(kind, args.grid)
        sc = Scene(args.grid, flags, vel, kw)
        for _ in range(3):
            print(kind, sc.solve(PcMGStatic), flush=True)
        sc.plugins.releaseMG(sc.s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build", "parent", "libmanta_hip_parent.so"))
    ap.add_argument("--step", choices=["time", "profile"], help="(internal) run one step in this process")
    args = ap.parse_args()
    args.out_dir = os.path.abspath(args.out_dir)
    args.parent_lib = os.path.abspath(args.parent_lib)
    if args.step == "time":
        return step_time(args)
    if args.step == "profile":
        return step_profile(args)
    if not os.path.exists(args.parent_lib):
        sys.exit("mg_time.py: %s not found (see the module docstring for how to build the parent's library)" % args.parent_lib)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--grid", str(args.grid), "--reps", str(args.reps), "--out-dir", args.out_dir,
          "--parent-lib", args.parent_lib]
    rc = subprocess.call(["timeout", "-k", "10", "420"] + me + ["--step", "time"])
    if rc != 0:
        sys.exit("mg_time.py: the timing step ended with status %d; nothing more is run" % rc)
    for tag, env in (("", {}), ("_cgonly", {"MF_MG_TAIL_VERTS": "0"})):
        tdir = os.path.join(args.out_dir, "_mg_trace" + tag)
        shutil.rmtree(tdir, ignore_errors=True)
        rc = subprocess.call(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "-o", "mg",
                              "--"] + me + ["--step", "profile"], env=dict(os.environ, **env))
        if rc != 0:
            sys.exit("mg_time.py: the profiling step ended with status %d; nothing more is run" % rc)
        found = glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            sys.exit("mg_time.py: rocprofv3 wrote no kernel statistics under %s" % tdir)
        shutil.copy(found[0], os.path.join(args.out_dir, "mg_kernel_stats%s.csv" % tag))
        shutil.rmtree(tdir, ignore_errors=True)
    print("mg_time.py: wrote mg_time.json, mg_kernel_stats.csv, mg_kernel_stats_cgonly.csv to", args.out_dir)


if __name__ == "__main__":
    main()
