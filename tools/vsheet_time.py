"""Per-call times of the vortex-sheet plugins on a createMesh sheet: a sphere of radius 0.3 * n in an n^3 grid (64 and 128 by default).
Timed: vorticitySource without and with the velocity pair (the second forms the acceleration grid), smoothVorticity(iter=3) with warm
connectivity tables, its weight table and its three passes alone through the library entries, texcoordInflow with a box of an eighth of
the grid and with a box of 8^3 cells, meshSmokeInflow, calcVorticity and reinitTexCoords.  Median, minimum and maximum of --calls calls after --warmup; every timed
window ends in a device synchronise; the host clock is around one call, so launch and Python overhead are inside.  The mesh size is
recorded beside the timings.  VICintegration(sigma=1.5, precondition=2) is timed whole, its spreading alone and its three solves alone,
with the CG iterations; the --stats table splits the spreading into pass A (k_spread_tri) and pass B (k_spread_cell).

Prints one JSON line and writes it to <out>/vsheet_time.json.  With --stats, a child process first runs the calls of the largest size
under `rocprofv3 --kernel-trace --stats` (a run of its own, before this process opens the GPU); its kernel table becomes
<out>/vsheet_kernel_stats.csv and the rows of this extension's kernels go into the JSON line.

  python tools/vsheet_time.py [--warmup 5] [--calls 10] [--sizes 64:128] [--out profiles] [--stats]
"""
import argparse
import csv
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


def _stats(a):
    import numpy as np
    a = np.asarray(a)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def sheet(m, vs, n):
    import numpy as np
    s = m.Solver(name="sphere", gridSize=m.vec3(n, n, n), dim=3)
    s.timestep = 0.5
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    c = 0.5 * n
    phi = s.create(m.LevelsetGrid)
    phi.from_numpy((np.sqrt((x + 0.5 - c) ** 2 + (y + 0.5 - c) ** 2 + (z + 0.5 - c) ** 2) - 0.3 * n).astype(np.float32))
    mesh = s.create(vs.VortexSheetMesh)
    phi.createMesh(mesh)
    return s, mesh


def time_sheet(m, vs, torch, s, mesh, n, warmup, calls):
    import numpy as np

    def timed(fn):
        ts = []
        for r in range(warmup + calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return _stats(ts)

    nt = mesh.numTris()
    out = {"grid": list(s.mGridSize), "nodes": mesh.numNodes(), "triangles": nt, "warmup_calls": warmup, "timed_calls": calls}
    r = np.random.RandomState(7)
    mesh.set_sheet_numpy(vorticity=r.uniform(-1, 1, (nt, 3)), circulation=r.uniform(-1, 1, (nt, 3)))
    vel, old = s.create(m.MACGrid), s.create(m.MACGrid)
    for g in (vel, old):
        g.data.copy_(torch.from_numpy(r.uniform(-1, 1, g.data.numel()).astype(np.float32)).to(g.data.device))
    gravity = m.vec3(0, -0.5, 0)
    out["vorticitySource_ms"] = timed(lambda: vs.vorticitySource(mesh, gravity, scale=0.01, mult=0.99))
    out["vorticitySource_with_vel_ms"] = timed(lambda: vs.vorticitySource(mesh, gravity, vel, old, scale=0.01, mult=0.99))
    mesh.corners_numpy()
    out["smoothVorticity_iter3_ms"] = timed(lambda: vs.smoothVorticity(mesh, iter=3))
    conn, lib, ch = mesh._conn, s.lib, mesh._channels("vsheet_time")
    w, t0, t1 = (torch.empty(3 * nt, dtype=torch.float32, device=s.device) for _ in range(3))
    idx = torch.empty(3 * nt, dtype=torch.int32, device=s.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out["smooth_weights_entry_ms"] = timed(lambda: lib.call("mf_vsheet_smooth_weights", *(mesh._mesh_args() + (p(conn["opposite"]), -12.5, p(w), p(idx),
                                                                                                             s.stream))))
    out["smooth_3_passes_entry_ms"] = timed(lambda: lib.call("mf_vsheet_smooth_iterate", nt, mesh.tcap, p(w), p(idx), 3, 0.8, p(ch["vorticity"]),
                                                            p(ch["vorticitySmoothed"]), p(t0), p(t1), s.stream))
    # VICintegration: the whole call, the spreading alone (its two passes are split in the --stats kernel table: k_spread_tri is pass A,
    # k_spread_cell pass B), and the three solves alone from the spread vorticity
    flags = s.create(m.FlagGrid)
    flags.initDomain(boundaryWidth=1)
    flags.fillGrid()
    vvel, vvort = s.create(m.MACGrid), s.create(m.VecGrid)
    out["VICintegration_ms"] = timed(lambda: vs.VICintegration(mesh, 1.5, vvel, flags, vorticity=vvort, precondition=2))
    out["VICintegration_cg"] = vs.lastVortexSheetStats()["vic"]
    need = ctypes.c_int64(0)
    lib.call("mf_vsheet_spread_tmp_bytes", n, n, n, 1.5, nt, ctypes.byref(need))
    stmp = torch.empty(need.value, dtype=torch.uint8, device=s.device)
    wn = torch.empty(nt, dtype=torch.float32, device=s.device)
    out["VIC_spreading_ms"] = timed(lambda: lib.call("mf_vsheet_spread", n, n, n, flags.ptr, *(mesh._mesh_args() + (p(ch["vorticity"]), 1.5, p(wn),
                                                                                                                     vvort.ptr, p(stmp), need.value, s.stream))))
    out["VIC_three_solves_ms"] = timed(lambda: vs._vic_solve(lib, s, vvort, vvel, flags, 1.5, 1e-3, 0.01))
    box = m.Box(parent=s, p0=m.vec3(0.25 * n, 0.25 * n, 0.25 * n), p1=m.vec3(0.75 * n, 0.75 * n, 0.75 * n))
    out["inflow_cells"] = int(np.asarray(box._inside_centres(s)).sum())
    vs.resetVortexSheetState()
    out["texcoordInflow_ms"] = timed(lambda: vs.texcoordInflow(mesh, box, vel))
    small = m.Box(parent=s, p0=m.vec3(0.5 * n - 4, 0.5 * n - 4, 0.5 * n - 4), p1=m.vec3(0.5 * n + 4, 0.5 * n + 4, 0.5 * n + 4))
    out["inflow_cells_small"] = int(np.asarray(small._inside_centres(s)).sum())
    out["texcoordInflow_small_ms"] = timed(lambda: vs.texcoordInflow(mesh, small, vel))
    vs.resetVortexSheetState()
    out["meshSmokeInflow_ms"] = timed(lambda: vs.meshSmokeInflow(mesh, box, 0.5))
    out["calcVorticity_ms"] = timed(mesh.calcVorticity)
    out["reinitTexCoords_ms"] = timed(mesh.reinitTexCoords)
    return out


def kernel_stats(out_dir, size):
    """the traced child's kernel table, copied to out_dir; returns the rows of this extension's kernels"""
    tmp = tempfile.mkdtemp(prefix="vsheet_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--sizes", size, "--warmup", "1", "--calls", "3", "--no-write"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        dst = os.path.join(out_dir, "vsheet_kernel_stats.csv")
        shutil.copyfile(found[0], dst)
        with open(dst) as f:
            return [row for row in csv.DictReader(f) if any(k in row.get("Name", "") for k in ("vsheet", "k_inflow", "k_spread", "k_bin_starts", "k_curl", "k_rhs", "k_set_component"))]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sizes", default="64:128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--stats", action="store_true", help="also record the rocprofv3 kernel table of the largest size (a child process, run first)")
    ap.add_argument("--no-write", action="store_true", help="print only (what the traced child does)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    rows = kernel_stats(args.out, str(max(int(x) for x in args.sizes.split(":")))) if args.stats else None
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vsheet_time.py needs a GPU")
    import manta as m
    from mantaflow_amd import vortexsheet as vs
    out = {"gpu": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (int(x) for x in args.sizes.split(":")):
        s, mesh = sheet(m, vs, n)
        torch.cuda.synchronize()
        out["sizes"][str(n)] = time_sheet(m, vs, torch, s, mesh, n, args.warmup, args.calls)
        del s, mesh
        torch.cuda.empty_cache()
    if rows is not None:
        out["kernel_stats"] = rows
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "vsheet_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
