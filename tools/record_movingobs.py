"""Recorder of tests/golden/movingobs.npz: the reference's outputs for the cases of tests/movingobs_model.py (inputs are regenerated
from its seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.
Everything derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP
thread (REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmovingobs_rec.so tools/movingobs_record.cpp -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_movingobs.py $B/libmovingobs_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Before anything is written the recorder asserts that the numpy model reproduces every recorded array bit for bit.

Two things in the reference are per process.  FlagGrid::mark_surface fills its neighbour list on the first call, for that solver's
dimension, so the 2-D grids are recorded by a child process (this script with --surf2d).  KnProjectParticles' random stream is never
reseeded, so the projections are recorded once, in the order of movingobs_model.PROJECT_SEQUENCE, and by nothing else in this process.

What the reference cannot record: it is the NOPYTHON packaging, in which MovingObstacle::moveLinear throws "Not yet supported..." at
its first applyToGrid.  For an obstacle with a shape the file holds what happened before that: move/<case>/states (the shapes after
setCenter(pos), i.e. the eased position) and move/<case>/reset_flags.  Calls with alpha outside [0, 1] and obstacles without a shape
run to the end: move/<case>/flags and move/<case>/vel.  The stamping of the shapes, v and the velocity pass are the model's alone; the
recorder stores the model's result as move/<case>/model_flags and move/<case>/model_vel and says so in the key.

Keys: wall2/<g>, bound/<g>/r<rule>/w<w>, surf/<g>/<kind>, clear/<g>/b<0|1>, cnorm/<g>/<real|vec|mac>/v<q>, reset/<g>, extrap/<g>/o<0|1>,
extrap/<g>/plain (phiObs = None), setters/<q>/{state, centre}, ids/{ids, threw, after}, ids/message, move/<case>/..., proj/<q>,
with <g> a grid of movingobs_model.DIMS.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import movingobs_model as M  # noqa: E402

f32 = np.float32


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def C(a, dt=f32):
    return np.ascontiguousarray(a, dt)


def same(tag, got, want):
    assert M.same(got, want), "%s: the model differs from the reference (%d elements)" % (tag, M.differing(np.asarray(got), np.asarray(want)))


def opener(libpath):
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())
    return call


def record_surf(call, out, names):
    for name in names:
        for kind in M.SURF_KINDS:
            f = C(M.surf_input(name, kind), np.int32)
            want = M.mark_surface(f)
            call("rec_mark_surface", *M.DIMS[name], P(f))
            same("surf/%s/%s" % (name, kind), want, f)
            out["surf/%s/%s" % (name, kind)] = f


def record_grids(call, out):
    for name, dims in M.DIMS.items():
        f, v, o = M.wall2_inputs(name)
        want = M.set_wall_bcs2(f, v, o)
        v = C(v)
        call("rec_set_wall_bcs2", *dims, P(C(f, np.int32)), P(v), P(C(o)))
        same("wall2/" + name, want, v)
        out["wall2/" + name] = v

        for rule in (0, 1, 2):
            for w in M.BOUND_WIDTHS:
                v = C(M.bound_input(name))
                want = M.set_bound_mac(v, M.BOUND_VALUE, w, rule)
                call("rec_set_bound_mac", *dims, P(v), fc(M.BOUND_VALUE[0]), fc(M.BOUND_VALUE[1]), fc(M.BOUND_VALUE[2]), w, rule)
                key = "bound/%s/r%d/w%d" % (name, rule, w)
                same(key, want, v)
                out[key] = v

        for b in (0, 1):
            f = C(M.clear_input(name), np.int32)
            want = M.clear_obstacle(f, bool(b))
            call("rec_clear_obstacle", *dims, P(f), b)
            key = "clear/%s/b%d" % (name, b)
            same(key, want, f)
            out[key] = f

        for kind, code in (("real", 0), ("vec", 1), ("mac", 2)):
            for q, val in enumerate(M.CNORM_VALS):
                a = C(M.cnorm_input(name, "real" if kind == "real" else "vec"))
                want = M.clamp_norm(a, val)
                call("rec_clamp_norm", code, *dims, P(a), fc(val))
                key = "cnorm/%s/%s/v%d" % (name, kind, q)
                same(key, want, a)
                out[key] = a

        f, phi = M.reset_inputs(name)
        want = M.reset_phi_in_obs(f, phi)
        phi = C(phi)
        call("rec_reset_phi_in_obs", *dims, P(C(f, np.int32)), P(phi))
        same("reset/" + name, want, phi)
        out["reset/" + name] = phi

        for into in (0, 1):
            f, v, phi, _ = M.extrap_inputs(name)
            want = M.extrapolate_mac_simple(f, v, M.EXTRAP_DISTANCE, phi, bool(into))
            v = C(v)
            call("rec_extrapolate", *dims, P(C(f, np.int32)), P(v), M.EXTRAP_DISTANCE, P(C(phi)), into)
            key = "extrap/%s/o%d" % (name, into)
            same(key, want, v)
            out[key] = v
        f, v, phi, _ = M.extrap_inputs(name)
        want = M.extrapolate_mac_simple(f, v, M.EXTRAP_DISTANCE, None, False)
        v = C(v)
        call("rec_extrapolate", *dims, P(C(f, np.int32)), P(v), M.EXTRAP_DISTANCE, None, 0)
        same("extrap/%s/plain" % name, want, v)
        out["extrap/%s/plain" % name] = v
        assert not M.same(out["extrap/%s/plain" % name], out["extrap/%s/o0" % name])
        print("grids", name, "done")


def record_setters(call, out):
    for q, (kind, args, centre, doCyl, r, z) in enumerate(M.SETTER_CASES):
        state, c3 = np.zeros(8, f32), np.zeros(3, f32)
        call("rec_shape_setters", kind, P(C(args)), P(C(centre)), doCyl, fc(r), P(C(z)), P(state), P(c3))
        ws, wc = M.setters_model(kind, args, centre, doCyl, r, z)
        same("setters/%d/state" % q, ws, state)
        same("setters/%d/centre" % q, wc, c3)
        out["setters/%d/state" % q], out["setters/%d/centre" % q] = state, c3
    print("setters done")


def record_ids(call, out):
    ids = np.zeros(7, np.int32)
    threw, after = ctypes.c_int(-9), ctypes.c_int(-9)
    msg = ctypes.create_string_buffer(256)
    call("rec_ids", 7, P(ids), ctypes.byref(threw), msg, ctypes.byref(after))
    assert list(ids[:5]) == [1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14] and threw.value == 5 and after.value == 17, (ids, threw.value, after.value)
    out["ids/ids"], out["ids/threw"], out["ids/after"] = ids, np.array([threw.value], np.int32), np.array([after.value], np.int32)
    out["ids/message"] = np.frombuffer(msg.value.split(b"\n")[0], np.uint8).copy()      # the first line: the second names the source file
    print("ids", ids, threw.value, after.value, msg.value.decode())


def record_moves(call, out):
    for case, c in M.move_cases().items():
        dims = M.DIMS[c["grid"]]
        f, v = M.move_inputs(case)
        f, v = C(f, np.int32), C(v)
        n = len(c["shapes"])
        kinds = C([k for k, _ in c["shapes"]] or [0], np.int32)
        args = C([a for _, a in c["shapes"]] or [[0] * 8])
        states = np.zeros((max(n, 1), 8), f32)
        threw = ctypes.c_int(-9)
        msg = ctypes.create_string_buffer(256)
        call("rec_move", *dims, fc(M.MOVE_DT), c["which"], c["emptyType"], n, P(kinds), P(args), fc(c["t"]), fc(c["t0"]), fc(c["t1"]), P(C(c["p0"])),
             P(C(c["p1"])), c["smooth"], P(f), P(v), P(states), ctypes.byref(threw), msg)
        states = states[:n]
        f0, v0 = M.move_inputs(case)
        mf, mv, ms = M.move_model(case)
        eased = M.ease(c["t"], c["t0"], c["t1"], c["p0"], c["p1"], M.MOVE_DT, bool(c["smooth"]))
        same("move/%s/states" % case, ms, states)
        out["move/%s/states" % case] = states
        if threw.value:
            assert n > 0 and eased is not None and msg.value.decode().startswith("Not yet supported..."), (case, msg.value)
            same("move/%s/reset_flags" % case, M.move_reset(f0, M.move_id(c["which"]), c["emptyType"]), f)
            same("move/%s: vel before the velocity pass" % case, v0, v)
            out["move/%s/reset_flags" % case] = f
            out["move/%s/model_flags" % case], out["move/%s/model_vel" % case] = mf, mv          # the MODEL's, not a recording
        else:
            assert n == 0 or eased is None, case
            same("move/%s/flags" % case, mf, f)
            same("move/%s/vel" % case, mv, v)
            out["move/%s/flags" % case], out["move/%s/vel" % case] = f, v
        print("move", case, "threw" if threw.value else "ran to the end", "cells changed", int((f != f0).sum()))


def record_projections(call, out):
    stream = M.Stream()
    for q, (what, name, n) in enumerate(M.PROJECT_SEQUENCE):
        dims = M.DIMS[name]
        pos, flag = M.particles(name, n, what)
        want = M.project_step(q, stream)
        pos, flag = C(pos), C(flag, np.int32)
        if what == "grad":
            call("rec_project", *dims, P(C(M.gradient_input(name))), n, P(pos), P(flag))
        else:
            call("rec_obstacle_project", *dims, P(C(M.obstacle_flags(name), np.int32)), n, P(pos), P(flag))
        same("proj/%d" % q, want, pos)
        out["proj/%d" % q] = pos
        print("projection", q, what, name, n, "reals drawn so far", stream.drawn)
    assert not M.same(out["proj/3"], out["proj/4"])


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    call = opener(libpath)
    out = {}
    record_surf(call, out, [n for n, d in M.DIMS.items() if d[2] > 1])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "surf2d.npz")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), libpath, "--surf2d", path])
        with np.load(path) as z:
            for k in z.files:
                out[k] = z[k]
    record_grids(call, out)
    record_setters(call, out)
    record_ids(call, out)
    record_moves(call, out)
    record_projections(call, out)
    np.savez_compressed(M.GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (M.GOLDEN, len(out), os.path.getsize(M.GOLDEN)))
    assert os.path.getsize(M.GOLDEN) < 1000000


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[2] == "--surf2d":
        res = {}
        record_surf(opener(sys.argv[1]), res, [n for n, d in M.DIMS.items() if d[2] == 1])
        np.savez(sys.argv[3], **res)
    else:
        main(sys.argv[1])
