"""Recorder of tests/golden/mesh.npz, tests/golden/mesh_small.obj and tests/golden/mesh_small.bobj.gz: the reference's outputs for the
fixture cases of tests/mesh_model.py (inputs are regenerated from its seeded generators, never stored) and for the recorded FLIP loop.
No test runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays
in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch
directory outside the tree):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so (levelset.cpp, mesh.cpp and fileio/iomeshes.cpp are part of it)
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmesh_rec.so tools/mesh_record.cpp -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_mesh.py $B/libmesh_rec.so $B

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Arrays of more than mesh_model.FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha.  Before anything is written
the recorder asserts that the numpy model reproduces every recorded array bit for bit, and that the cases meet the conditions they
exist for (from the model's counters; asserted again in tests/test_mesh_model.py).  The rotation scalars are the C library's sinf / cosf
as the package's library returns them on the recording machine.
"""
import ctypes
import gzip
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_model as M  # noqa: E402

f32, i64 = np.float32, ctypes.c_int64


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    u = "u%d" % got.dtype.itemsize
    d = got.view(u) != want.view(u)
    assert not d.any(), "%s: the model differs from the reference in %d of %d words, first at %s (%r vs %r)" % (
        tag, int(d.sum()), d.size, np.argwhere(d)[0], got[tuple(np.argwhere(d)[0])], want[tuple(np.argwhere(d)[0])])


def ref_create(call, phi):
    sz, sy, sx = phi.shape
    n = phi.size
    counts = np.zeros(2, np.int64)
    pos, nrm, tris = np.zeros((3 * n, 3), f32), np.zeros((3 * n, 3), f32), np.zeros((5 * n, 3), np.int32)
    call("rec_create_mesh", sx, sy, sz, P(phi), i64(3 * n), i64(5 * n), P(counts), P(pos), P(nrm), P(tris))
    return {"pos": pos[:counts[0]].copy(), "normal": nrm[:counts[0]].copy(), "tris": tris[:counts[1]].copy()}


def record_create(call, out):
    cnt = {}
    for name in M.all_cases():
        phi = M.case_phi(name)
        ref = ref_create(call, phi)
        model, c = M.model_mesh(name)
        for k in ("pos", "normal", "tris"):
            if name.startswith("cfg") and k == "tris" and (model[k].shape != ref[k].shape or not np.array_equal(model[k], ref[k])):
                raise AssertionError("configuration %s: the model's triangles differ from the reference's:\n%s\n%s" % (name, model[k], ref[k]))
            same("create/%s/%s" % (name, k), model[k], ref[k])
        M.put_mesh(out, "create/" + name, ref)
        for k, v in c.items():
            cnt[k] = cnt.get(k, 0) + v
        if not name.startswith("cfg"):
            print("create", name, ref["pos"].shape[0], "nodes", ref["tris"].shape[0], "triangles", c)
    print("createMesh counters:", cnt)
    for k in ("norm_one", "norm_scaled", "norm_zero", "owner_passed", "iso_exact"):
        assert cnt.get(k, 0) > 0, k
    assert M.model_mesh("invalid")[1]["owner_passed"] > 0 and M.model_mesh("rand33")[1]["owner_passed"] > 0
    assert M.model_mesh("pos")[0]["pos"].shape[0] == 0 and M.model_mesh("neg")[0]["tris"].shape[0] == 0
    phi2d = np.zeros((1, 4, 4), f32)
    try:
        ref_create(call, phi2d)
        raise AssertionError("a 2-D grid did not raise")
    except RuntimeError as e:
        assert "Only 3D grids supported so far" in str(e), str(e)


def record_vnorm(call, out):
    for name in M.VNORM_CASES:
        pos, tris = M.vnorm_inputs(name)
        nrm = np.full(pos.shape, 7, f32)
        call("rec_vertex_normals", i64(pos.shape[0]), P(np.ascontiguousarray(pos)), i64(tris.shape[0]), P(np.ascontiguousarray(tris)), P(nrm))
        same("vnorm/" + name, M.vertex_normals(pos, tris), nrm)
        M.put(out, "vnorm/" + name, nrm)
        print("vnorm", name, "zero normals:", int((nrm == 0).all(1).sum()), "NaN:", int(np.isnan(nrm).any(1).sum()))


def record_files(call, out, scratch):
    gold = os.path.join(ROOT, "tests", "golden")
    mesh = M.model_mesh(M.SAVE_CASE)[0]
    sx, sy, sz = M.SAVE_DIMS
    n, t = mesh["pos"].shape[0], mesh["tris"].shape[0]
    for ext in ("obj", "bobj.gz"):
        path = os.path.join(scratch, "mesh_small." + ext)
        nrm = mesh["normal"].copy()
        call("rec_save", sx, sy, sz, i64(n), P(mesh["pos"]), P(nrm), i64(t), P(mesh["tris"]), path.encode())
        want = mesh["normal"] if ext == "obj" else M.vertex_normals(mesh["pos"], mesh["tris"])
        same("save/%s/normal_after" % ext, want, nrm)
        M.put(out, "save/%s/normal_after" % ext, nrm)
        shutil.copyfile(path, os.path.join(gold, "mesh_small." + ext))
        for append, pre in ((0, 0), (0, 2), (1, 2)):
            if ext == "bobj.gz" and append:
                try:
                    ref_load(call, path, append, pre, n, t)
                    raise AssertionError("append did not raise")
                except RuntimeError as e:
                    assert "append not yet implemented" in str(e), str(e)
                    out["msg/bobj_append"] = np.frombuffer(str(e).split("\n")[0].encode(), np.uint8)
                continue
            m = ref_load(call, path, append, pre, n, t)
            M.put_mesh(out, "load/%s/%d%d" % (ext, append, pre), m)
            print("load", ext, append, pre, m["pos"].shape[0], m["tris"].shape[0], "normals all zero:", bool((m["normal"][pre if append else 0:] == 0).all()))
    for name in ("noext", "mesh.txt"):
        try:
            ref_load(call, os.path.join(scratch, name), 0, 0, 1, 1)
            raise AssertionError("did not raise")
        except RuntimeError as e:
            msg = str(e).split("\n")[0].replace(scratch + os.sep, "")        # the first line: the second names the reference's source file
            out["msg/load_" + name] = np.frombuffer(msg.encode(), np.uint8)
            print("message:", msg)


def ref_load(call, path, append, pre, n, t):
    capN, capT = n + pre + 4, t + 4
    counts = np.zeros(2, np.int64)
    pos, nrm, tris = np.zeros((capN, 3), f32), np.zeros((capN, 3), f32), np.zeros((capT, 3), np.int32)
    sx, sy, sz = M.SAVE_DIMS
    call("rec_load", sx, sy, sz, path.encode(), append, pre, i64(capN), i64(capT), P(counts), P(pos), P(nrm), P(tris))
    return {"pos": pos[:counts[0]].copy(), "normal": nrm[:counts[0]].copy(), "tris": tris[:counts[1]].copy()}


def record_advect(call, out):
    sx, sy, sz = M.ADV_DIMS
    for n in M.ADV_SIZES:
        vel, pos, nflags = M.advect_inputs(n)
        for mode in (0, 1, 2):
            p = pos.T.copy()
            call("rec_advect", sx, sy, sz, fc(M.ADV_DT), P(vel), i64(n), P(p), P(nflags), mode)
            model = M.advect_nodes(M.ADV_DIMS, vel, pos, nflags, M.ADV_DT, mode)
            same("adv/%d/%d" % (n, mode), np.ascontiguousarray(model.T), p)
            M.put(out, "adv/%d/%d" % (n, mode), p)
            if n == 5000 and mode == 2:
                moved = (p != pos.T).any(1)
                fixed = (nflags & 1) != 0
                print("advect: %d of %d nodes moved, %d fixed" % (moved.sum(), n, fixed.sum()))
                assert moved.any() and not moved[fixed].any() and (~moved & ~fixed).any()


def record_transform(call, out):
    from mantaflow_amd import core, _lib
    import util
    lib = _lib.Library(_lib.DEFAULT_LIB, "cpu")
    assert lib.mesh
    pos = M.xf_inputs()
    for key, op, v in (("scale", 0, M.XF_SCALE), ("offset", 1, M.XF_OFFSET), ("savepos", 3, M.XF_SCALE)):
        p = pos.copy()
        call("rec_transform", op, i64(p.shape[0]), P(p), fc(v[0]), fc(v[1]), fc(v[2]))
        v32 = np.array(v, f32)
        same("xf/" + key, {"scale": pos * v32, "offset": pos + v32, "savepos": pos}[key], p)
        M.put(out, "xf/" + key, p)
    for q, th in enumerate(M.ROT_THETAS):
        p = pos.copy()
        call("rec_transform", 2, i64(p.shape[0]), P(p), fc(th[0]), fc(th[1]), fc(th[2]))
        sc = np.array([core._c_sincos(lib, float(f32(t))) for t in th], f32)
        same("xf/rotate/%d" % q, np.ascontiguousarray(M.rotate(np.ascontiguousarray(pos.T), th, sc).T), p)
        M.put(out, "xf/rotate/%d" % q, p)
        out["xf/rotate/%d/scalars" % q] = sc
    try:
        call("rec_load_pos_changed")
        raise AssertionError("load_pos did not raise")
    except RuntimeError as e:
        assert "# of mesh nodes has changed" in str(e)
        out["msg/load_pos"] = np.frombuffer(str(e).split("\n")[0].encode(), np.uint8)
        print("message:", str(e).split("\n")[0])


def record_loop(call, out):
    res, steps = M.LOOP_RES, M.LOOP_STEPS
    n = res ** 3
    counts, crc = np.zeros((steps, 2), np.int64), np.zeros(steps, np.uint32)
    capN, capT = n, 2 * n
    pos, nrm, tris, adv = np.zeros((capN, 3), f32), np.zeros((capN, 3), f32), np.zeros((capT, 3), np.int32), np.zeros((capN, 3), f32)
    call("rec_loop_mesh", res, steps, M.LOOP_ADV_STEPS, P(counts), P(crc), i64(capN), i64(capT), P(pos), P(nrm), P(tris), P(adv))
    nn, nt = counts[-1]
    print("loop: nodes / triangles per step", counts.tolist())
    assert (counts > 0).all() and len(set(counts[:, 0].tolist())) > 1
    out["loop/counts"], out["loop/crc"] = counts, crc
    M.put_mesh(out, "loop/mesh", {"pos": pos[:nn].copy(), "normal": nrm[:nn].copy(), "tris": tris[:nt].copy()})
    assert (adv[:nn] != pos[:nn]).any()
    M.put(out, "loop/adv", adv[:nn].copy())


def main(libpath, scratch):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    record_create(call, out)
    record_vnorm(call, out)
    record_files(call, out, scratch)
    record_advect(call, out)
    record_transform(call, out)
    record_loop(call, out)
    path = M.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
