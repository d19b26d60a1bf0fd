"""Recorder of tests/golden/meshsdf.npz: the reference's Mesh::computeLevelset for every case of tests/meshsdf_model.py (inputs are
regenerated from its seeded generators and the two .obj fixtures, never stored), its densityInflowMesh for one of them and the loop of
scenes/meshload.py at a small size.  No test runs
this; it needs the reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch
directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory outside
the tree):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so (mesh.cpp and plugin/initplugins.cpp are part of it)
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmeshsdf_rec.so tools/meshsdf_record.cpp -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_meshsdf.py $B/libmeshsdf_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Per case the fixture holds the SHA-256 of the reference's field, the cells in which it is not bit-identical to the model's (indices and
values: the model's field with those patched in is the reference's, which the digest proves), their number, and the field itself where
it has at most meshsdf_model.FULL_LIMIT cells.  Before anything is written the recorder asserts, per case: the conditions that go with
the tolerance (no pre-flood value of the model within its bound of cutoff - 1 or of 0), that every differing cell is a written,
unflooded cell within the bound, and therefore that the flooded set, the written set and every sign equal the reference's.  The
reference's applyMeshToGrid is compiled out under NOPYTHON: its kernel is pinned through computeLevelset plus the model's element-wise
statement.  The loop of scenes/meshload.py is recorded on the torus at res 24 for 6 steps (flags, CG iterations per step, the
final density, velocity and pressure).  densityInflowMesh is recorded directly; densityInflowMeshNoise is pinned through
computeLevelset(sigma = 1) plus the package's existing densityInflow kernel.

With --time <out.json> it instead times the reference's computeLevelset, single-threaded as it is written, on the meshes of
tools/meshsdf_time.py and writes them under the key `reference_cpu`.
"""
import ctypes
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshsdf_model as M  # noqa: E402

f32, i64 = np.float32, ctypes.c_int64


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ref_levelset(call, c):
    pos, tris = np.ascontiguousarray(c["pos"], f32), np.ascontiguousarray(c["tris"], np.int32)
    phi = np.zeros(int(np.prod(c["dims"])), f32)
    sec = ctypes.c_double(0)
    call("rec_compute_levelset", *c["mesh_gs"], i64(pos.shape[0]), P(pos), i64(tris.shape[0]), P(tris), *c["dims"], ctypes.c_float(c["sigma"]),
         ctypes.c_float(c["cutoff"]), P(phi), ctypes.byref(sec))
    return phi, sec.value


def record(call):
    out = {}
    for name in M.CASES:
        c, R = M.case(name), M.model(name)
        ref, _ = ref_levelset(call, c)
        assert M.margin_ok(R), "%s: a pre-flood value of the model lies within its bound of cutoff - 1 or of 0" % name
        model, cut = R["phi"], R["P"]["cutoff"]
        d = np.nonzero(ref.view(np.uint32) != model.view(np.uint32))[0]
        flooded = R["phi"].view(np.uint32) != R["pre"].view(np.uint32)
        b = M.bound(R["C"], ref)
        assert R["C"]["written"][d].all() and not flooded[d].any(), "%s: a cell that is not a written, unflooded one differs" % name
        err = np.abs(ref[d].astype(np.float64) - model[d])
        assert (err <= b[d]).all(), "%s: %d cells beyond the bound, worst %g of its bound" % (name, int((err > b[d]).sum()), (err / b[d]).max())
        assert np.array_equal(ref == cut, model == cut) and np.array_equal(ref < 0, model < 0) and not np.isnan(ref).any(), name
        out[name + "/sha"] = M.sha(ref)
        out[name + "/diff_idx"], out[name + "/diff_val"] = d.astype(np.int64), ref[d]
        out[name + "/ndiff"] = np.array([d.size, int(R["C"]["written"].sum())], np.int64)
        if ref.size <= M.FULL_LIMIT:
            out[name + "/phi"] = ref
        print("%-16s %6d cells, %5d written, %5d flooded, %4d not bit-identical to the model (worst %.3f of the bound)"
              % (name, ref.size, R["counters"]["written"], R["counters"]["flooded"], d.size, (err / b[d]).max() if d.size else 0.0))
    # the cases exist for these
    cnt = {n: M.model(n)["counters"] for n in M.CASES}
    assert cnt["faces"]["dropped"] == 5 and cnt["faces"]["binned"] == 5 and cnt["zero_area"]["norm_zero"] == 2
    assert cnt["span"]["sources"] > 4000 and cnt["dense"]["max_in_cell"] >= 200 and cnt["outside"]["binned"] == 0
    for k, big in M.BIG_EXPECT.items():
        for sfx in "sl":
            assert M.tri_plan(M.case(k + sfx)["pos"])[0] == big, (k, sfx)
    assert cnt["sphere_open"]["flooded"] > cnt["sphere_closed"]["flooded"] + 1000
    # densityInflowMesh
    name = M.INFLOW_CASE
    c = M.case(name)
    flags, dens = M.inflow_inputs(name)
    for q, (value, cutoff, sigma) in enumerate(M.INFLOW_ARGS):
        got = dens.copy()
        pos, tris = np.ascontiguousarray(c["pos"], f32), np.ascontiguousarray(c["tris"], np.int32)
        call("rec_density_inflow_mesh", *c["dims"], i64(pos.shape[0]), P(pos), i64(tris.shape[0]), P(tris), P(flags), P(got),
             ctypes.c_float(value), ctypes.c_float(cutoff), ctypes.c_float(sigma))
        want = M.inflow_model(name, q)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "densityInflowMesh %d: the model differs in %d cells" % (
            q, int((got != want).sum()))
        assert (got != dens).any() and (got == dens).any()
        out["inflow/%d/sha" % q] = M.sha(got)
        print("densityInflowMesh", q, "cells set:", int((got != dens).sum()))
    # the loop of scenes/meshload.py on the torus at res 24
    c = M.case(M.LOOP_CASE)
    res, n = c["dims"][0], int(np.prod(c["dims"]))
    pos, tris = np.ascontiguousarray(c["pos"], f32), np.ascontiguousarray(c["tris"], np.int32)
    cyl = M.loop_cylinder(res)
    flags, iters = np.zeros(n, np.int32), np.zeros(M.LOOP_STEPS, np.int32)
    dens, vel, pres = np.zeros(n, f32), np.zeros(3 * n, f32), np.zeros(n, f32)
    call("rec_meshload_loop", res, M.LOOP_STEPS, i64(pos.shape[0]), P(pos), i64(tris.shape[0]), P(tris), P(cyl), P(flags), P(iters), P(dens),
         P(vel), P(pres))
    assert (iters > 0).all() and (dens > 0).any() and np.abs(vel).max() > 0 and np.isfinite(vel).all()
    inner = np.zeros(c["dims"][::-1], bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert np.array_equal(((flags & 2) != 0)[inner.reshape(-1)], (M.model(M.LOOP_CASE)["phi"] < 0)[inner.reshape(-1)])
    out["loop/flags"], out["loop/iterations"] = flags.astype(np.int16), iters
    out["loop/density"], out["loop/vel"], out["loop/pressure"] = dens, vel, pres
    print("meshload loop: CG iterations per step", iters.tolist(), "obstacle cells", int(((flags & 2) != 0).sum()), "max |vel| %g" % np.abs(vel).max())
    np.savez_compressed(M.GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (M.GOLDEN, len(out), os.path.getsize(M.GOLDEN)))


def time_reference(call, path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import meshsdf_time as T
    res = {"machine": "%s, %d CPUs, one thread" % (platform.processor() or platform.machine(), os.cpu_count()), "unit": "seconds", "calls": {}}
    for key, (fname, r, shift) in T.WORKLOADS.items():
        p, t = M.load_obj(os.path.join(M.GOLD, fname))
        c = M._case((r, r, r), M.obj_placed(p, r, shift), t)
        secs = [ref_levelset(call, c)[1] for _ in range(3 if r <= 128 else 1)]
        res["calls"][key] = {"median": float(np.median(secs)), "min": min(secs), "max": max(secs), "runs": len(secs)}
        print(key, res["calls"][key], flush=True)
    data = json.load(open(path)) if os.path.exists(path) else {}
    data["reference_cpu"] = res
    json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def main(argv):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(argv[1])
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    if len(argv) > 3 and argv[2] == "--time":
        time_reference(call, argv[3])
    else:
        record(call)


if __name__ == "__main__":
    main(sys.argv)
