"""Per-call times of the mesh operations on createMesh meshes: the liquid surface of scenes/flip01_simple.py's loop at 128^3 and of
scenes/benchmark_dam.py's at 379x356x124 (the states of tools/mesh_time.py, phi from unionParticleLevelset), and a sphere of radius
0.3 * n in an n^3 grid, which is closed whatever the liquid states are.  Timed: the connectivity build alone (the tables dropped before
every call), one smoothMesh step with warm tables, a whole smoothMesh(steps=10), and killSmallComponents with its labelling rounds.
Median, minimum and maximum of --calls calls after --warmup; every timed window ends in a device synchronise; the host clock is
around one call, so launch and Python overhead are inside.  Mesh sizes and the counts of edge groups are recorded beside the timings.

A mesh with an edge that only one triangle uses is refused by the connectivity build, as the reference refuses it
("can't rebuild corners, index without an opposite"); the build is still timed there (it runs to its read-back), the number of such
edges is recorded, and smoothMesh and killSmallComponents are reported as refused, not timed.  killSmallComponents is timed on a
copy of the mesh per call (the copy is outside the window); where nothing is small enough to go it times the plan alone.

Prints one JSON line and writes it to <out>/meshops_time.json.  `reference_cpu` is filled by hand from
`tools/record_meshops.py <lib> <scratch> --time`, which runs the reference single-threaded on spheres small enough for its
quadratic corner search.

  python tools/meshops_time.py [--warmup 5] [--calls 10] [--states sphere48:sphere128:flip01:dam] [--out profiles]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _stats(a):
    import numpy as np
    a = np.asarray(a)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def sphere_mesh(m, n):
    import numpy as np
    s = m.Solver(name="sphere", gridSize=m.vec3(n, n, n), dim=3)
    s.timestep = 0.5
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    c = 0.5 * n
    phi = s.create(m.LevelsetGrid)
    phi.from_numpy((np.sqrt((x + 0.5 - c) ** 2 + (y + 0.5 - c) ** 2 + (z + 0.5 - c) ** 2) - 0.3 * n).astype(np.float32))
    mesh = s.create(m.Mesh)
    phi.createMesh(mesh)
    return s, mesh


def liquid_mesh(m, name):
    import mesh_time
    st = {"flip01": mesh_time.flip01_state, "dam": mesh_time.dam_state}[name](m)
    s, flags, pp = st["s"], st["flags"], st["parts"]
    pindex, gpi, phi, mesh = s.create(m.ParticleIndexSystem), s.create(m.IntGrid), s.create(m.LevelsetGrid), s.create(m.Mesh)
    m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
    m.unionParticleLevelset(pp, pindex, flags, gpi, phi)
    phi.createMesh(mesh)
    return s, mesh


def time_mesh(m, torch, s, mesh, warmup, calls):
    def timed(fn, before=None):
        ts = []
        for r in range(warmup + calls):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        return _stats(ts)

    out = {"grid": list(s.mGridSize), "nodes": mesh.numNodes(), "triangles": mesh.numTris(), "warmup_calls": warmup, "timed_calls": calls}

    def drop():
        mesh._conn = None

    def build():
        try:
            mesh.corners_numpy()
        except RuntimeError as e:
            out["refused"] = str(e)
    build()
    st = m.lastMeshOpsStats()
    out["edge_groups_of_one"], out["edge_groups_of_three_or_more"] = st["singletons"], st["multi"]
    lib = s.lib

    def build_only():                                  # without corners_numpy's copy of the table to the host
        try:
            mesh._connectivity(lib, "meshops_time")
        except RuntimeError:
            pass
    out["connectivity_ms"] = timed(build_only, before=drop)
    if "refused" in out:
        out["smoothMesh"] = out["killSmallComponents"] = "refused with the mesh: " + out["refused"]
        return out
    mesh.save_pos()
    out["smooth_1_step_warm_tables_ms"] = timed(lambda: m.smoothMesh(mesh, 0.6, 1), before=mesh.load_pos)
    out["smooth_10_steps_ms"] = timed(lambda: m.smoothMesh(mesh, 0.6, 10), before=mesh.load_pos)
    mesh.load_pos()
    if st["multi"]:
        out["killSmallComponents"] = "refused with the mesh: killSmallComponents: non-manifold edge"
        return out
    pos, normal, nflags = mesh.nodes_numpy()
    tris, tflags = mesh.tris_numpy()
    work = s.create(m.Mesh)

    def reset():
        work.set_numpy(pos, normal, nflags, tris, tflags)
        work.corners_numpy()                           # warm tables: the window holds the labelling, the plan and the removal
    out["kill_ms"] = timed(lambda: m.killSmallComponents(work), before=reset)
    k = m.lastMeshOpsStats()
    out["kill"] = {"rounds": k["rounds"], "components": k["components"], "tris_deleted": k["tris"], "nodes_deleted": k["nodes"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--states", default="sphere48:sphere128:flip01:dam")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("meshops_time.py needs a GPU")
    import manta as m
    out = {"gpu": torch.cuda.get_device_name(0), "states": {}, "reference_cpu": None}
    for name in args.states.split(":"):
        s, mesh = sphere_mesh(m, int(name[6:])) if name.startswith("sphere") else liquid_mesh(m, name)
        torch.cuda.synchronize()
        out["states"][name] = time_mesh(m, torch, s, mesh, args.warmup, args.calls)
        del s, mesh
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "meshops_time.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
