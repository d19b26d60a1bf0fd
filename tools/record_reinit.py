"""Recorder of tests/golden/reinit.npz: the reference's LevelsetGrid::reinitMarching for every case of tests/reinit_model.py (inputs are
regenerated from its seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of
oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with
one OpenMP thread (REF: the reference checkout, B: any scratch directory outside the tree):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so (levelset.cpp and fastmarch.cpp are part of it)
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libreinit_rec.so tools/reinit_record.cpp -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_reinit.py $B/libreinit_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

The loops of tools/tests/test_2050_freesurface.py (24^3 for 8 steps, 32x32 for 12) and test_2045_fallingDrop.py (20^3 for 6) are
recorded as CG iterations per step, the final phi and vel, the digest of the level set the shapes give, and per step whether the model's
march in rounds flags on the input the reference's loop hands to reinitMarching.

Per case the fixture holds the reference's phi and vel -- the arrays themselves up to reinit_model.FULL_LIMIT elements, their SHA-256
beyond -- and, from the model, the FastMarch flags and keys as the outward march leaves them (the reference keeps them to itself) and the
counters of the march in rounds (windows, sub-rounds, pops, serial; inward and outward).  Before anything is written the recorder asserts
that the model's serial statement and its statement in rounds both give the reference's bits, and the same flags and keys as each other.

With --time <out.json> it instead times the reference's reinitMarching, one thread, on the inputs that tools/reinit_time.py dumped and
writes the figures under the key `reference_cpu`.
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
import reinit_model as M  # noqa: E402

f32 = np.float32


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def ref_reinit(call, dims, phi, flags, vel, maxTime, ignoreWalls, correctOuterLayer, obstacleType):
    phi = np.ascontiguousarray(phi, f32).copy()
    vel = None if vel is None else np.ascontiguousarray(vel, f32).copy()
    sec = ctypes.c_double(0)
    call("rec_reinit", *dims, P(phi), P(np.ascontiguousarray(flags, np.int32)), P(vel), ctypes.c_float(maxTime), int(ignoreWalls),
         int(correctOuterLayer), int(obstacleType), ctypes.byref(sec))
    return phi, vel, sec.value


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def put(out, key, a):
    if a.size <= M.FULL_LIMIT:
        out[key] = a
    else:
        out[key + "_sha"] = np.array(M.sha(a))


def record(call):
    out = {}
    for name in M.CASES:
        c = M.case(name)
        phi, vel, _ = ref_reinit(call, c["dims"], c["phi"], c["flags"], c["velocity"], c["maxTime"], c["ignoreWalls"], c["correctOuterLayer"],
                                 c["obstacleType"])
        S, R = M.model(name, "serial"), M.model(name, "rounds")
        for tag, r in (("serial", S), ("rounds", R)):
            assert same(r["phi"], phi), "%s: the model's %s statement differs from the reference in %d cells" % (
                name, tag, int((r["phi"].view(np.uint32) != phi.view(np.uint32)).sum()))
            assert vel is None or same(r["vel"], vel), "%s: the model's %s statement differs from the reference's velocity" % (name, tag)
        assert np.array_equal(S["fm"], R["fm"]) and same(S["key"], R["key"]), name
        put(out, name + "/phi", phi)
        if vel is not None:
            put(out, name + "/vel", vel)
        put(out, name + "/fm", R["fm"].astype(np.int8))
        put(out, name + "/key", R["key"])
        out[name + "/stats"] = np.array([R["stats"][k] for k in ("windows", "subrounds", "pops", "serial")], np.int64)
        print("%-22s %6d cells  windows %-9s sub-rounds %-9s pops %-14s serial %s" % (
            name, c["n"], R["stats"]["windows"], R["stats"]["subrounds"], R["stats"]["pops"], R["stats"]["serial"]), flush=True)
    # the loops of test_2050_freesurface.py and test_2045_fallingDrop.py
    for name, (dims, steps, scene) in M.LOOPS.items():
        n = int(np.prod(dims))
        iters, phi0, phi, vel = np.zeros(steps, np.int32), np.zeros(n, f32), np.zeros(n, f32), np.zeros(3 * n, f32)
        phi_in, flags_in, vel_in = np.zeros((steps, n), f32), np.zeros((steps, n), np.int32), np.zeros((steps, 3 * n), f32)
        call("rec_liquid_loop", *dims, steps, scene, P(iters), P(phi0), P(phi), P(vel), P(phi_in), P(flags_in), P(vel_in))
        assert (iters > 0).all() and np.isfinite(vel).all() and np.abs(vel).max() > 0
        serial = []
        for t in range(steps):          # what the model's march in rounds does with each step's input: it must be the reference's result
            R = M.call(dims, phi_in[t], flags_in[t], vel_in[t], 4.0)
            want = ref_reinit(call, dims, phi_in[t], flags_in[t], vel_in[t], 4.0, False, True, 2)
            assert same(R["phi"], want[0]) and same(R["vel"], want[1]), (name, t)
            serial.append(R["stats"]["serial"])
        out["loop/%s/iterations" % name], out["loop/%s/serial" % name] = iters, np.array(serial, np.int8)
        out["loop/%s/phi0_sha" % name] = np.array(M.sha(phi0))
        out["loop/%s/phi" % name], out["loop/%s/vel" % name] = phi, vel
        print("loop %-6s %s %d steps: CG iterations %s, marches the model redoes serially %s" % (name, dims, steps, iters.tolist(),
                                                                                                np.array(serial).sum(0).tolist()), flush=True)
    np.savez_compressed(M.GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (M.GOLDEN, len(out), os.path.getsize(M.GOLDEN)))


def time_reference(call, path):
    data = json.load(open(path)) if os.path.exists(path) else {}
    res = {"machine": "%s, %d CPUs, one thread" % (platform.processor() or platform.machine(), os.cpu_count()), "unit": "seconds", "calls": {}}
    for key, w in sorted(data.get("inputs", {}).items()):
        a = np.load(os.path.join(os.path.dirname(path), w["file"]))
        dims = tuple(int(x) for x in a["dims"])
        secs = [ref_reinit(call, dims, a["phi"], a["flags"], a["vel"], 4.0, False, True, 2)[2] for _ in range(3)]
        res["calls"][key] = {"median": float(np.median(secs)), "min": min(secs), "max": max(secs), "runs": len(secs)}
        print(key, res["calls"][key], flush=True)
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
