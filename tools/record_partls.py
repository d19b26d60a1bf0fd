"""Recorder of tests/golden/partls.npz: the reference's outputs for the fixture cases of tests/partls_model.py (inputs are
regenerated from its seeded generators, never stored) and for the two recorded FLIP loops.  No test runs this; it needs the
reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory
outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so (plugin/flip.cpp is part of it)
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libpartls_rec.so tools/partls_record.cpp -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_partls.py $B/libpartls_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Per fixture case the file holds <case>/phi, and for the improved cases with smoothing <case>/stage: the same call with
smoothen = smoothenNeg = 0.  Per loop: iters, crc (crc32 of phi right after the level-set plugin, per step), phi, vel, pos, np.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import partls_model as M  # noqa: E402


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p
    i64, f32c = ctypes.c_int64, ctypes.c_float

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    def levelset(c, I, smoothen, smoothenNeg):
        sx, sy, sz = c["dims"]
        phi = np.full((sz, sy, sx), 123.0, np.float32)
        pos = np.ascontiguousarray(I["pos"].T, np.float32)
        pflag = np.ascontiguousarray(I["pflag"], np.int32)
        pt = None if I["ptype"] is None else np.ascontiguousarray(I["ptype"], np.int32)
        nidx = i64(0)
        call("rec_levelset", sx, sy, sz, i64(len(pflag)), P(pos), P(pflag), None if pt is None else P(pt), int(I["exclude"]), int(c["improved"]),
             f32c(c["radiusFactor"]), smoothen, smoothenNeg, f32c(c["t_low"]), f32c(c["t_high"]), P(phi), ctypes.byref(nidx))
        return phi, nidx.value

    out = {}
    for name, c in M.CASES.items():
        I = M.case_inputs(name)
        out[name + "/phi"], nidx = levelset(c, I, c["smoothen"], c["smoothenNeg"])
        if c["improved"] and (c["smoothen"] or c["smoothenNeg"]):
            out[name + "/stage"], _ = levelset(c, I, 0, 0)
        print(name, "particles", len(I["pflag"]), "indexed", nidx)
    res, steps = M.LOOP_RES, M.LOOP_STEPS
    n = res ** 3
    for name, cfg in M.LOOPS.items():
        cap = 16 * n
        iters, crc = np.zeros(steps, np.int64), np.zeros(steps, np.uint32)
        phi, vel, pos = np.zeros((res, res, res), np.float32), np.zeros((3, n), np.float32), np.zeros((3, cap), np.float32)
        npo = i64(0)
        call("rec_loop", int(cfg["improved"]), res, steps, P(iters), P(crc), P(phi), P(vel), i64(cap), P(pos), ctypes.byref(npo))
        out[name + "/iters"], out[name + "/crc"], out[name + "/phi"] = iters, crc, phi
        out[name + "/vel"] = np.ascontiguousarray(vel.T.reshape(res, res, res, 3))
        out[name + "/pos"] = np.ascontiguousarray(pos[:, :npo.value].T)[::M.LOOP_EVERY]
        out[name + "/np"] = np.array([npo.value], np.int64)
        print(name, "iters", iters, "np", npo.value)
    path = os.path.join(ROOT, "tests", "golden", "partls.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
