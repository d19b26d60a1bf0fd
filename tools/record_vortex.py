"""Recorder of tests/golden/vortex.npz: the reference's outputs for the cases of tests/vortex_model.py (inputs are regenerated from its
seeded generators, never stored) and for the recorded seeding / advection loop.  No test runs this; it needs the reference checkout and
the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU
machine with one OpenMP thread (REF: the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/vortexplugins.cpp $B/plugin/vortexplugins.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libvortex_rec.so $B/plugin/vortexplugins.cpp tools/vortex_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_vortex.py $B/libvortex_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction; tools/vortex_record.cpp includes the expanded
vortexpart.cpp from $PP for its two velocity kernels)

Arrays of more than vortex_model.FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha.  Before anything is written
the recorder asserts that the numpy model reproduces every recorded array bit for bit (the loop excepted: it goes through advectInGrid,
which has its own fixtures), so a digest in the file is the digest of an array the model can regenerate.

All VPseedK41 cases run in this one process in the fixed order SEED_ORDER and the loop after them, because the random stream is a static
of the reference.  The file holds vel/<case>/u, end/<case>/<mode>, seed/<case>/{pos, vorticity, sigma, flag, cursors}, density/<case>,
fixed/<exclusive>, loop/{pos, vorticity, sigma, flag, sizes, start}.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vortex_model as M  # noqa: E402

f32, i64 = np.float32, ctypes.c_int64


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def C(a, dtype):
    return np.ascontiguousarray(a, dtype)


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    u = "u%d" % got.dtype.itemsize
    d = got.view(u) != want.view(u)
    assert not d.any(), "%s: the model differs from the reference in %d of %d words, first at %s (%r vs %r)" % (
        tag, int(d.sum()), d.size, np.argwhere(d)[0], got[tuple(np.argwhere(d)[0])], want[tuple(np.argwhere(d)[0])])


def shape_args(shape):
    if shape[0] == "box":
        return 0, np.array(shape[1], f32), np.array(shape[2], f32)
    return 1, np.array(shape[1], f32), np.array([shape[2]] * 3, f32)


def record_kernel(call, out):
    cnt = {}
    for name in M.CASES:
        I = M.case_inputs(name)
        S = I["P"]
        nS = S["pos"].shape[0]
        sp, sv, ss, sf = C(S["pos"], f32), C(S["vorticity"], f32), C(S["sigma"], f32), C(S["flag"], np.int32)
        tp, tz = M.case_targets(I)
        nT = tp.shape[0]
        u = np.full((nT, 3), 7, f32)
        dt = f32(0.5)                      # the methods take scale and multiply by dt: scale * dt is the case's factor
        scale = f32(I["scale"] / dt)
        assert f32(scale * dt) == I["scale"]
        if I["kind"] == "self":
            call("rec_velocity", 1, i64(0), None, None, i64(nS), P(sp), P(sv), P(ss), P(sf), fc(I["scale"]), P(u))
        else:
            tf = C(I["nflags"], np.int32)
            call("rec_velocity", 0, i64(nT), P(C(tp, f32)), P(tf), i64(nS), P(sp), P(sv), P(ss), P(sf), fc(I["scale"]), P(u))
        same("vel/%s" % name, M.case_velocity(name, cnt), u)
        M.put(out, "vel/%s/u" % name, u)
        for mode in M.MODES:
            if I["kind"] == "self":
                x = sp.copy()
                call("rec_advect_self", i64(nS), P(x), P(sv), P(ss), P(sf), fc(scale), fc(dt), mode)
            else:
                x = C(tp, f32).copy()
                call("rec_apply_to_mesh", i64(nT), P(x), P(tf), i64(nS), P(sp), P(sv), P(ss), P(sf), fc(scale), fc(dt), mode)
            same("end/%s/%d" % (name, mode), M.run_case(name, mode), x)
            M.put(out, "end/%s/%d" % (name, mode), x)
        print("case", name, "done")
    print("kernel counters:", cnt)
    for key in ("at_cutoff_kept", "ulp_beyond_cutoff", "coincident", "rho2_small", "branch_zero", "branch_unit", "branch_scaled", "sigma_zero",
                "underflow", "deleted_sources", "zeroed_targets", "inside"):
        assert cnt.get(key, 0) > 0, key


def record_seed(L, call, out):
    res = M.run_seed_cases()
    for name in M.SEED_ORDER:
        dims, dt, calls = M.SEED_CASES[name]
        call("rec_seed_open", dims[0], dims[1], dims[2], fc(dt))
        for c in calls:
            kind, a, b = shape_args(c[0])
            call("rec_seed_call", kind, P(a), P(b), *[fc(v) for v in c[1:]])
        n = int(L.rec_seed_size())
        cap = max(n, 1)
        pos, vort, sig, fl = np.zeros((cap, 3), f32), np.zeros((cap, 3), f32), np.zeros(cap, f32), np.zeros(cap, np.int32)
        call("rec_seed_read", i64(cap), P(pos), P(vort), P(sig), P(fl))
        ref = dict(pos=pos[:n], vorticity=vort[:n], sigma=sig[:n], flag=fl[:n])
        model, start, end = res[name]
        for ch in M.CHANNELS:
            same("seed/%s/%s" % (name, ch), model[ch], ref[ch])
            M.put(out, "seed/%s/%s" % (name, ch), ref[ch])
        out["seed/%s/cursors" % name] = np.array([start, end], np.int64)
        print("seed", name, "particles", n, "stream", start, "->", end)
    call("rec_seed_close")
    return res[M.SEED_ORDER[-1]][2]


def record_rest(call, out):
    for name in M.DENSITY_CASES:
        phi, value, sigma = M.density_inputs(name)
        sz, sy, sx = phi.shape
        d = np.full(phi.shape, 9, f32)
        call("rec_density", sx, sy, sz, P(phi), P(d), fc(value), fc(sigma))
        same("density/%s" % name, M.density_from_levelset(phi, value, sigma), d)
        M.put(out, "density/%s" % name, d)
    pos, flags = M.fixed_inputs()
    for ex in (0, 1):
        fl = flags.copy()
        call("rec_mark_as_fixed", i64(len(fl)), P(pos), P(fl), P(np.array(M.FIXED_BOX[1], f32)), P(np.array(M.FIXED_BOX[2], f32)), ex)
        same("fixed/%d" % ex, M.mark_as_fixed(pos, flags, M.FIXED_BOX, bool(ex)), fl)
        out["fixed/%d" % ex] = fl


def record_loop(call, out, cursor):
    C_ = M.LOOP
    sx, sy, sz = C_["dims"]
    flags, vel = M.loop_grids()
    soa = np.ascontiguousarray(vel.reshape(-1, 3).T)
    steps, cap = C_["steps"], 4096
    sizes = np.zeros(steps, np.int64)
    pos, vort, sig, fl = np.zeros((cap, 3), f32), np.zeros((cap, 3), f32), np.zeros(cap, f32), np.zeros(cap, np.int32)
    n = i64(0)
    call("rec_loop", sx, sy, sz, fc(C_["dt"]), steps, P(flags), P(soa), P(np.array(C_["shape"][1], f32)), fc(C_["shape"][2]), fc(C_["strength"]),
         fc(C_["sigma0"]), fc(C_["sigma1"]), fc(C_["probability"]), fc(C_["N"]), fc(C_["scale"]), P(sizes), i64(cap), ctypes.byref(n),
         P(pos), P(vort), P(sig), P(fl))
    m = n.value
    print("loop: sizes per step", sizes, "after compress", m)
    assert 0 < m < sizes[-1], "the loop deletes nothing (or everything)"
    out["loop/sizes"] = np.concatenate([sizes, [m]])
    out["loop/start"] = np.array([cursor], np.int64)
    for key, a in (("pos", pos[:m]), ("vorticity", vort[:m]), ("sigma", sig[:m]), ("flag", fl[:m])):
        M.put(out, "loop/" + key, a)


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p
    L.rec_seed_size.restype = ctypes.c_int64

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    cursor = record_seed(L, call, out)
    record_loop(call, out, cursor)
    record_rest(call, out)
    record_kernel(call, out)
    path = os.path.join(ROOT, "tests", "golden", "vortex.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
