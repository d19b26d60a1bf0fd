"""Recorder of tests/golden/idp.npz: the reference's outputs for the fixture cases of tests/idp_model.py (inputs are regenerated
from its seeded generators, never stored) and for the two recorded scene loops.  No test runs this; it needs the reference
checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside
the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/implicitdensityprojection.cpp $B/plugin/implicitdensityprojection.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libidp_rec.so $B/plugin/implicitdensityprojection.cpp tools/idp_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_idp.py $B/libidp_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import idp_model as M  # noqa: E402


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def soa(g):
    """[z][y][x][3] -> [3][n]"""
    return np.ascontiguousarray(np.asarray(g, np.float32).reshape(-1, 3).T)


def aos(a, shape):
    return np.ascontiguousarray(a.reshape(3, -1).T.reshape(shape + (3,)))


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p
    i64, f32c = ctypes.c_int64, ctypes.c_float

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    for name, (kind, dims, seed, opt) in M.CASES.items():
        sx, sy, sz = dims
        shape = (sz, sy, sx)
        I = M.case_inputs(name)
        if kind in ("mark", "mass"):
            flags = np.ascontiguousarray(I["flags"], np.int32).copy()
            dX = np.zeros((3, sx * sy * sz), np.float32)
            phi = np.ascontiguousarray(I["phiObs"], np.float32)
            pos = np.ascontiguousarray(I["pos"].T, np.float32)
            pflag = np.ascontiguousarray(I["pflag"], np.int32)
            n = i64(len(pflag))
            if kind == "mark":
                pt = np.ascontiguousarray(I["ptype"], np.int32) if opt["ptype"] else None
                call("rec_mark", sx, sy, sz, P(flags), P(dX), P(phi), n, P(pos), P(pflag), P(pt) if pt is not None else None,
                     I["exclude"] if opt["ptype"] else 0)
            else:
                dens = np.zeros(shape, np.float32)
                call("rec_map_mass", sx, sy, sz, P(flags), P(dens), P(dX), P(phi), n, P(pos), P(pflag), f32c(I["dt"]), f32c(I["mass"]),
                     int(opt["noClamp"]))
                out[name + "/density"] = dens
            out[name + "/flags"] = flags
            out[name + "/deltaX"] = aos(dX, shape)
        elif kind == "delta":
            dX = soa(I["deltaX"])
            Lm = np.ascontiguousarray(I["Lambda"], np.float32).copy()
            call("rec_compute_delta_x", sx, sy, sz, P(dX), P(Lm), P(np.ascontiguousarray(I["flags"], np.int32)))
            out[name + "/deltaX"] = aos(dX, shape)
            out[name + "/Lambda"] = Lm
        else:
            pos = np.ascontiguousarray(I["pos"].T, np.float32).copy()
            pt = np.ascontiguousarray(I["ptype"], np.int32) if opt["ptype"] else None
            call("rec_map_positions", sx, sy, sz, P(soa(I["deltaX"])), i64(len(I["pflag"])), P(pos), P(np.ascontiguousarray(I["pflag"], np.int32)),
                 f32c(I["dt"]), P(pt) if pt is not None else None, I["exclude"] if opt["ptype"] else 0)
            out[name + "/pos"] = np.ascontiguousarray(pos.T)
    for name, cfg in M.LOOPS.items():
        res, dim, steps = cfg["res"], cfg["dim"], cfg["steps"]
        shape = (res if dim == 3 else 1, res, res)
        n = res * res * shape[0]
        cap = 64 * n
        per = np.zeros((steps, 3), np.float32)
        dens, lam = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        dX, vel = np.zeros((3, n), np.float32), np.zeros((3, n), np.float32)
        fl, flp = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        pos = np.zeros((3, cap), np.float32)
        npo = i64(0)
        call("rec_loop", res, dim, steps, f32c(cfg["cfl"]), P(per), P(dens), P(lam), P(dX), P(vel), P(fl), P(flp), i64(cap), P(pos), ctypes.byref(npo))
        out[name + "/dt"] = per[:, 0].copy()
        out[name + "/it_pos"] = per[:, 1].astype(np.int64)
        out[name + "/it_vel"] = per[:, 2].astype(np.int64)
        out[name + "/density"], out[name + "/Lambda"], out[name + "/flags"], out[name + "/flagsPos"] = dens, lam, fl, flp
        out[name + "/deltaX"], out[name + "/vel"] = aos(dX, shape), aos(vel, shape)
        out[name + "/pos"] = np.ascontiguousarray(pos[:, :npo.value].T)[::M.LOOP_EVERY]
        out[name + "/np"] = np.array([npo.value], np.int64)
        print(name, "dt", per[:, 0], "it_pos", per[:, 1], "it_vel", per[:, 2], "np", npo.value)
    path = os.path.join(ROOT, "tests", "golden", "idp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
