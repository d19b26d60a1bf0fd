"""Times of the z-slab form of the multigrid preconditioner at world 1 on one GPU, by the protocol of tools/mg_time.py: medians of
alternating runs in one process, so clocks and cache state are shared.  The yardstick is the undivided V-cycle of the same build.
  * one cut-form V-cycle (slab.SlabMG.vcycle: the ranged level-0 passes of include/open/manta_hip_mgslab.h, the replicated
    levels, the copy in and out of the slab's grids; at world 1 the exchanges and the gather move nothing) against one
    mf_mg_vcycle ON THE SAME HANDLE, by device events
  * one slab.solvePressure(PcMGStatic) in steady state (hierarchy kept) against the plugin solvePressure(PcMGStatic) with the
    options the slab path takes, by the host clock around a synchronised solve
Input: the liquid input of tools/mg_time.py (util.make_flags(seed 1, obstacle blobs, empty top third), smooth velocity), max-norm
accuracy 1e-4 -- the slab path has no zero-pressure fixing, and the multigrid does not converge on the singular closed box.
More than one GPU cannot be measured here: the multi-GPU speed of this route is unmeasured.

  python tools/mgslab_time.py [--grid 256] [--reps 7] [--out-dir profiles]
Writes <out-dir>/mgslab_time.json.  The timing runs in a child process under its own time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ACCURACY = 1e-4


def stats(xs):
    xs = sorted(xs)
    return dict(median_ms=round(xs[len(xs) // 2], 4), min_ms=round(xs[0], 4), max_ms=round(xs[-1], 4), n=len(xs))


def step_time(args):
    import ctypes
    import torch
    import cases
    import mg_time
    from mantaflow_amd import core, plugins, slab
    assert torch.cuda.is_available(), "mgslab_time.py needs a GPU"
    n = args.grid
    dims = (n, n, n)
    flags_g, vel_g, _ = mg_time.inputs("liq", n)
    # the slab route at world 1, and a plain solver for the plugin route
    dom = slab.SlabDomain(dims, slab.required_ghost(2.0))
    s = dom.solver
    flags, vel, vel0, pres = core.FlagGrid(s), core.MACGrid(s), core.MACGrid(s), core.Grid(s)
    dom.scatter_global(flags, flags_g); dom.scatter_global(vel0, vel_g)
    slab.setWallBcs(dom, flags, vel0)
    sg = cases._mk_solver(dims)
    fg, vg, vg0, pg = core.FlagGrid(sg), core.MACGrid(sg), core.MACGrid(sg), core.Grid(sg)
    cases.soa_to_grid(fg, flags_g); cases.soa_to_grid(vg0, vel_g)
    plugins.setWallBcs(fg, vg0)

    def slab_solve():
        vel.copyFrom(vel0)
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        slab.solvePressure(dom, vel, pres, flags, cgAccuracy=ACCURACY, stats=st, preconditioner=slab.PcMGStatic)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, st

    def plugin_solve():
        vg.copyFrom(vg0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plugins.solvePressure(vg, pg, fg, cgAccuracy=ACCURACY, preconditioner=plugins.PcMGStatic)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, plugins.lastCgStats()["iterations"]

    # warm-up of both routes (the first Static solve builds the hierarchy that the later ones keep)
    _, st = slab_solve()
    _, pit = plugin_solve()
    assert st["iterations"] == pit and torch.equal(pres.data, pg.data), "slab world 1 and the plugin disagree"
    t = dict(slab_static=[], plugin_static=[])
    for _ in range(args.reps):
        t["slab_static"].append(slab_solve()[0])
        t["plugin_static"].append(plugin_solve()[0])
    # one V-cycle, both forms on the slab domain's handle
    mg = dom._mg
    src, dst, whole = core.Grid(s), core.Grid(s), torch.zeros(n ** 3, dtype=torch.float32, device=s.device)
    dom.scatter_global(src, cases.cg_rhs(dims, flags_g, 7))
    cut = lambda: mg.vcycle(dst, src)
    und = lambda: s.lib.call("mf_mg_vcycle", mg.h.handle, ctypes.c_void_p(whole.data_ptr()), src.ptr, s.stream)
    cut(); und()
    torch.cuda.synchronize()
    assert torch.equal(dst.data, whole), "the cut form and mf_mg_vcycle disagree"
    v = dict(cut=[], undivided=[])
    for _ in range(max(args.reps, 20)):
        for name, call in (("cut", cut), ("undivided", und)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            v[name].append(e0.elapsed_time(e1))
    res = dict(grid=n, device=torch.cuda.get_device_name(0), reps=args.reps, world=1, accuracy=ACCURACY, iterations=st["iterations"],
               levels=st["mg_levels"], form=st["mg_form"], slab_static=stats(t["slab_static"]), plugin_static=stats(t["plugin_static"]),
               vcycle_cut=stats(v["cut"]), vcycle_undivided=stats(v["undivided"]))
    res["ratio_vcycle_cut_to_undivided"] = round(res["vcycle_cut"]["median_ms"] / res["vcycle_undivided"]["median_ms"], 3)
    res["ratio_solve_slab_to_plugin"] = round(res["slab_static"]["median_ms"] / res["plugin_static"]["median_ms"], 3)
    slab.releaseMG(dom)
    plugins.releaseMG(sg)
    with open(os.path.join(args.out_dir, "mgslab_time.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", choices=["time"], help="(internal) run the timing in this process")
    args = ap.parse_args()
    args.out_dir = os.path.abspath(args.out_dir)
    if args.step == "time":
        return step_time(args)
    os.makedirs(args.out_dir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--grid", str(args.grid), "--reps", str(args.reps), "--out-dir", args.out_dir]
    rc = subprocess.call(["timeout", "-k", "10", "420"] + me + ["--step", "time"])
    if rc != 0:
        sys.exit("mgslab_time.py: the timing step ended with status %d" % rc)
    print("mgslab_time.py: wrote mgslab_time.json to", args.out_dir)


if __name__ == "__main__":
    main()
