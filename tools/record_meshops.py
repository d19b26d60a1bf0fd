"""Recorder of tests/golden/meshops.npz and tests/golden/meshops_pipeline.bobj.gz: the reference's outputs for the fixture cases of
tests/meshops_model.py (inputs are regenerated from its seeded generators, never stored).  No test runs this; it needs the reference
checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside the tree.
Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory outside the tree):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/meshplugins.cpp $B/plugin/meshplugins.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmeshops_rec.so $B/plugin/meshplugins.cpp tools/meshops_record.cpp \\
        -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_meshops.py $B/libmeshops_rec.so $B

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Arrays of more than mesh_model.FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha.  Before anything is written
the recorder asserts that the numpy model reproduces every recorded array bit for bit.  For every smoothing case it also asserts that
the float scalars of the rescale (the two volumes, the two centres of mass, beta) are the same at every combination of the end points
of the reduction bound around the serial sums: the final positions then do not depend on the order in which the device adds the
volume terms.  killSmallComponents is recorded after Mesh::rebuildQuickCheck(), which the plugin itself does not call.

With --time as the third argument nothing is recorded: the reference's single-thread seconds for the connectivity build, one smoothMesh
step, smoothMesh(steps=10) and killSmallComponents on createMesh spheres of growing size are printed as one JSON object (the corner
search is quadratic; sizes above 8k triangles are skipped).
"""
import ctypes
import gzip
import itertools
import json
import os
import shutil
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_model as MM  # noqa: E402
import meshops_model as M  # noqa: E402

f32, f64, i32, i64 = np.float32, np.float64, np.int32, ctypes.c_int64
PIPE = {"res": 24, "dt": 0.5, "elements": 10, "strength": 0.6, "steps": 3}


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


def ref_connectivity(call, m, seconds=None):
    n, t = m["pos"].shape[0], m["tris"].shape[0]
    cap = max(6 * t, 1)
    opp, nodeOff, nodes = np.zeros(max(3 * t, 1), i32), np.zeros(n + 1, i32), np.zeros(cap, i32)
    triOff, tris = np.zeros(n + 1, i32), np.zeros(cap, i32)
    call("rec_connectivity", i64(n), P(m["pos"]), i64(t), P(m["tris"]), P(opp), P(nodeOff), P(nodes), P(triOff), P(tris), i64(cap), seconds)
    return {"opposite": opp[:3 * t].copy(), "nodeOff": nodeOff, "nodes": nodes[:nodeOff[n]].copy(), "triOff": triOff, "tris": tris[:triOff[n]].copy()}


def record_connectivity(call, out):
    for name, make in M.CONNECTIVITY_CASES.items():
        m = make()
        ref = ref_connectivity(call, m)
        model = M.connectivity("record", m)
        for k, v in ref.items():
            same("conn/%s/%s" % (name, k), model[k], v)
            M.put(out, "conn/%s/%s" % (name, k), v)
        print("connectivity", name, m["pos"].shape[0], "nodes", m["tris"].shape[0], "triangles, groups of three or more:", model["multi"])
    for name, (make, msg) in M.REFUSED_CASES.items():
        if name == "repeated":
            continue                                # the reference matches things that are not edges there; the package refuses
        try:
            ref_connectivity(call, make())
            raise AssertionError(name + " did not raise")
        except RuntimeError as e:
            first = str(e).split("\n")[0]
            assert first == msg, (first, msg)
            out["msg/" + name] = np.frombuffer(first.encode(), np.uint8)
            print("message:", first)


def endpoints_agree(terms0, terms1, s0, s1):
    """the float scalars of the rescale at all 2^8 combinations of sums -/+ bound"""
    b0, b1 = M.sum_bound(terms0), M.sum_bound(terms1)
    seen = set()
    for signs in itertools.product((-1.0, 1.0), repeat=8):
        sg = np.array(signs)
        a, b = s0 + sg[:4] * b0, s1 + sg[4:] * b1
        o, n, beta = M.rescale_scalars(a, b)
        seen.add(o.tobytes() + n.tobytes() + np.float32(beta).tobytes() + f32(a[0]).tobytes() + f32(b[0]).tobytes())
    return len(seen) == 1


def record_smooth(call, out):
    for name, make in M.SMOOTH_CASES.items():
        m, dt, strength, steps, minLength = make()
        n, t = m["pos"].shape[0], m["tris"].shape[0]
        pos, sums = m["pos"].copy(), np.zeros(4, f64)
        call("rec_smooth", fc(dt), i64(n), P(pos), P(m["flags"]), i64(t), P(m["tris"]), fc(strength), steps, fc(minLength), P(sums), None)
        model, msums = M.smooth_mesh(m, dt, strength, steps, minLength)
        same("smooth/%s/sums0" % name, msums[0], sums)
        same("smooth/%s/pos" % name, model["pos"], pos)
        # the positions between the steps and the rescale: the model's, which the final positions have just confirmed
        free = (m["flags"] & 1) == 0
        mid = M.copy_mesh(m)
        c = M.connectivity("record", m)
        str_ = min(f32(f32(dt) * f32(strength)), f32(1))
        for _ in range(steps):
            mid["pos"][free] = M.smooth_step(mid["pos"], c["nodeOff"], c["nodes"], c["triOff"], str_, f32(minLength))[free]
        assert endpoints_agree(M.volume_terms(m["pos"], m["tris"]), M.volume_terms(mid["pos"], m["tris"]), msums[0], msums[1]), name
        M.put(out, "smooth/%s/pos" % name, pos)
        out["smooth/%s/sums" % name] = msums
        print("smooth", name, n, "nodes, moved:", int((pos != m["pos"]).any(1).sum()), "beta:", M.rescale_scalars(msums[0], msums[1])[2])


def ref_kill(call, m, elements, seconds=None):
    n, t = m["pos"].shape[0], m["tris"].shape[0]
    r = M.copy_mesh(m)
    counts, text = np.zeros(2, np.int64), ctypes.create_string_buffer(256)
    call("rec_kill", i64(n), P(r["pos"]), P(r["normal"]), P(r["flags"]), i64(t), P(r["tris"]), P(r["tflags"]), elements, P(counts), text, i64(256), seconds)
    nn, nt = counts
    return {"pos": r["pos"][:nn].copy(), "normal": r["normal"][:nn].copy(), "flags": r["flags"][:nn].copy(), "tris": r["tris"][:nt].copy(),
            "tflags": r["tflags"][:nt].copy()}, text.value.decode()


def record_kill(call, out):
    for name, make in M.KILL_CASES.items():
        m, elements = make()
        ref, text = ref_kill(call, m, elements)
        model, stats = M.kill_small_components(m, elements)
        for k in M.MESH_KEYS:
            same("kill/%s/%s" % (name, k), model[k], ref[k])
        want = M.kill_message(stats) + "\n" if stats["tris"] else ""
        assert text == want, (text, want)
        M.put_mesh(out, "kill/" + name, ref)
        out["kill/%s/message" % name] = np.frombuffer(text.strip("\n").encode(), np.uint8)
        print("kill", name, "elements", elements, "->", ref["pos"].shape[0], "nodes", ref["tris"].shape[0], "triangles;", text.strip() or "nothing killed")


def record_pipeline(call, out, scratch):
    res = PIPE["res"]
    phi = M.two_blobs(res)
    path = os.path.join(scratch, "meshops_pipeline.bobj.gz")
    counts = np.zeros(4, np.int64)
    call("rec_pipeline", res, res, res, fc(PIPE["dt"]), P(phi), PIPE["elements"], fc(PIPE["strength"]), PIPE["steps"], path.encode(), P(counts))
    c = MM.create_mesh(phi)
    m = M.mesh(c["pos"], c["tris"], normal=c["normal"])
    assert (m["pos"].shape[0], m["tris"].shape[0]) == tuple(counts[:2]), counts
    killed, stats = M.kill_small_components(m, PIPE["elements"])
    assert 0 < stats["tris"] < 10 and stats["components"] == 2, stats
    final, _ = M.smooth_mesh(killed, PIPE["dt"], PIPE["strength"], PIPE["steps"])
    assert (final["pos"].shape[0], final["tris"].shape[0]) == tuple(counts[2:]), counts
    raw = gzip.open(path).read()
    n = struct.unpack_from("<i", raw, 0)[0]
    half = (np.full(3, res, f32).astype(f64) * 0.5).astype(f32)
    unit = (final["pos"] - half[None]) * f32(1.0 / res)
    want = struct.pack("<i", n) + unit.astype("<f4").tobytes() + struct.pack("<i", n) + MM.vertex_normals(final["pos"], final["tris"]).astype("<f4").tobytes() \
        + struct.pack("<i", final["tris"].shape[0]) + final["tris"].astype("<i4").tobytes()
    assert raw == want, "the model's pipeline differs from the reference's file"
    shutil.copyfile(path, os.path.join(ROOT, "tests", "golden", "meshops_pipeline.bobj.gz"))
    out["pipeline/counts"] = counts
    print("pipeline: nodes / triangles after createMesh and at the end", counts.tolist(), stats)


def time_reference(call):
    res = {}
    for r in (17, 24, 33, 48):
        m = M.sphere(r)
        t = m["tris"].shape[0]
        if t > 8192:
            res["sphere%d" % r] = {"triangles": t, "skipped": "the quadratic corner search"}
            continue
        sec = ctypes.c_double(0)
        row = {"nodes": m["pos"].shape[0], "triangles": t}
        ref_connectivity(call, m, ctypes.byref(sec))
        row["connectivity_s"] = sec.value
        for key, steps in (("smooth_1_step_s", 1), ("smooth_10_steps_s", 10)):
            pos, sums = m["pos"].copy(), np.zeros(4, f64)
            call("rec_smooth", fc(0.5), i64(m["pos"].shape[0]), P(pos), P(m["flags"]), i64(t), P(m["tris"]), fc(0.6), steps, fc(1e-5), P(sums), ctypes.byref(sec))
            row[key] = sec.value              # includes the plugin's own rebuildQuickCheck (the lookup exists, the corner table is built)
        ref_kill(call, M.join([m, M.tetrahedron(7, (1, 1, 1))]), 10, ctypes.byref(sec))
        row["kill_s"] = sec.value
        res["sphere%d" % r] = row
    print(json.dumps({"reference_cpu": res}))


def main(libpath, scratch, mode=None):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    if mode == "--time":
        return time_reference(call)
    out = {}
    record_connectivity(call, out)
    record_smooth(call, out)
    record_kill(call, out)
    record_pipeline(call, out, scratch)
    np.savez_compressed(M.GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (M.GOLDEN, len(out), os.path.getsize(M.GOLDEN)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
