"""Recorder of tests/golden/guiding.npz: the reference's results for the cases of tests/guiding_model.py (inputs are regenerated from
its seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything
derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread
(REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/fluidguiding.cpp $B/plugin/fluidguiding.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libguiding_rec.so $B/plugin/fluidguiding.cpp tools/guiding_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_guiding.py $B/libguiding_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

The file holds: weights/<r> for r = 0..16; <setup case>/out for the getSpiralVelocity / setGradientYWeight cases; per loop (a, b) and
per box run (c_cap, c_stop): pd (iterations per step), cg (CG iterations of every inner solve, in order), vel, pressure, density
(loops only); staged/{Q, invA, x, z_pre, z_post, y, rnorm, epsDual}: the box case taken apart, per iteration.  The conditions the
cases exist for are asserted here, on the reference alone.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guiding_model as M  # noqa: E402

MAX_ITERS = 200
CG_CAP = 4096


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
    f = ctypes.c_float

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    for r in M.RADII:
        w = np.zeros(2 * r + 1, np.float32)
        call("rec_weights", r, P(w))
        out["weights/%d" % r] = w
    for name, cfg in M.SETUP.items():
        (sx, sy, sz) = cfg[0]
        a = M.setup_input(name)
        if name.startswith("spiral"):
            v = soa(a)
            call("rec_spiral", sx, sy, sz, P(v), f(cfg[1]), int(cfg[2]))
            out[name + "/out"] = aos(v, (sz, sy, sx))
        else:
            a = np.ascontiguousarray(a)
            call("rec_gradient", sx, sy, sz, P(a), cfg[1], cfg[2], f(cfg[3]), f(cfg[4]))
            out[name + "/out"] = a

    # case (c) and its staged form
    B = M.BOX
    sx, sy, sz = B["dims"]
    shape = (sz, sy, sx)
    n = sx * sy * sz
    I = M.box_inputs()
    flags = np.ascontiguousarray(I["flags"], np.int32)
    W = np.ones(shape, np.float32)
    call("rec_gradient", sx, sy, sz, P(W), I["grad"][0], I["grad"][1], f(I["grad"][2]), f(I["grad"][3]))
    assert W.tobytes() == M.box_weight().tobytes(), "box_weight of the model differs from the reference's setGradientYWeight"
    for name, run in M.BOX_RUNS.items():
        vel, press = soa(I["vel"]), np.zeros(shape, np.float32)
        pd, cg, ncg = np.zeros(1, np.int32), np.zeros(CG_CAP, np.int32), ctypes.c_int32(0)
        call("rec_guiding", sx, sy, sz, P(flags), P(vel), P(soa(I["velT"])), P(press), P(W), B["blurRadius"], f(B["theta"]), f(B["tau"]),
             f(B["sigma"]), f(B["epsRel"]), f(run["epsAbs"]), run["maxIters"], B["preconditioner"], P(pd), P(cg), CG_CAP, ctypes.byref(ncg))
        out[name + "/pd"], out[name + "/cg"] = pd.astype(np.int64), cg[:ncg.value].astype(np.int64)
        out[name + "/vel"], out[name + "/pressure"] = aos(vel, shape), press
        print(name, "pd", pd, "cg", cg[:ncg.value])
    assert out["c_cap/pd"][0] == M.BOX_RUNS["c_cap"]["maxIters"] - 1, "c_cap must end at the cap"
    assert out["c_stop/pd"][0] == 1, "c_stop must end at iteration 1"
    iters = M.BOX_RUNS["c_cap"]["maxIters"]
    st = {k: np.zeros((iters, 3, n), np.float32) for k in ("x", "z_pre", "z_post", "y")}
    rn, ep = np.zeros(iters, np.float32), np.zeros(iters, np.float32)
    Q, invA = np.zeros((3, n), np.float32), np.zeros(shape, np.float32)
    call("rec_staged", sx, sy, sz, P(flags), P(soa(I["vel"])), P(soa(I["velT"])), P(W), B["blurRadius"], f(B["theta"]), f(B["tau"]), f(B["sigma"]),
         f(B["epsRel"]), f(M.BOX_RUNS["c_cap"]["epsAbs"]), B["preconditioner"], iters, P(st["x"]), P(st["z_pre"]), P(st["z_post"]), P(st["y"]),
         P(rn), P(ep), P(Q), P(invA))
    for k, v in st.items():
        out["staged/" + k] = np.stack([aos(v[i], shape) for i in range(iters)])
    out["staged/rnorm"], out["staged/epsDual"], out["staged/Q"], out["staged/invA"] = rn, ep, aos(Q, shape), invA
    assert out["staged/z_post"][-1].tobytes() == out["c_cap/vel"].tobytes(), "the staged loop is not the plugin's loop"
    assert not any(i > 0 and rn[i] < ep[i] for i in range(iters - 1)), "the staged case must not meet the criterion before the cap"

    for name, cfg in M.LOOPS.items():
        sx, sy, sz = cfg["dims"]
        shape = (sz, sy, sx)
        n = sx * sy * sz
        steps = cfg["steps"]
        vel, dens, press = np.zeros((3, n), np.float32), np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        pd, cg, ncg = np.zeros(steps, np.int32), np.zeros(CG_CAP, np.int32), ctypes.c_int32(0)
        if sz == 1:
            call("rec_loop_2d", sx, steps, cfg["scale"], cfg["blurRadius"], f(cfg["theta"]), f(cfg["tau"]), f(cfg["sigma"]), f(cfg["epsRel"]),
                 f(cfg["epsAbs"]), MAX_ITERS, cfg["preconditioner"], P(pd), P(cg), CG_CAP, ctypes.byref(ncg), P(vel), P(dens), P(press))
        else:
            call("rec_loop_3d", sx, steps, cfg["factor"], f(cfg["timestep"]), cfg["blurRadius"], f(cfg["wScalar"]), f(cfg["theta"]), f(cfg["tau"]),
                 f(cfg["sigma"]), f(cfg["epsRel"]), f(cfg["epsAbs"]), MAX_ITERS, cfg["preconditioner"], P(pd), P(cg), CG_CAP, ctypes.byref(ncg),
                 P(vel), P(dens), P(press))
        print(name, "pd", pd, "cg", cg[:ncg.value])
        assert all(0 < p < MAX_ITERS - 1 for p in pd), "loop %s must end by the criterion before the cap in every step: %s" % (name, pd)
        out[name + "/pd"], out[name + "/cg"] = pd.astype(np.int64), cg[:ncg.value].astype(np.int64)
        out[name + "/vel"], out[name + "/density"], out[name + "/pressure"] = aos(vel, shape), dens, press
    path = M.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
