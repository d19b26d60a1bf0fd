"""Recorder of tests/golden/datagen.npz: the reference's outputs for the cases of tests/datagen_model.py (inputs are regenerated from
its seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything
derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF:
the reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libdatagen_rec.so tools/datagen_record.cpp -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_datagen.py $B/libdatagen_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Before anything is written the recorder asserts that the numpy model reproduces every recorded array: blur, projection and Laplacian
bit for bit; curvature bit for bit as well (the model's fp64 pow is math.pow, the C library's, which is what the reference calls); the
centre of mass bit for bit where the sums are exact and within datagen_model.com_bound elsewhere, and the model's own statement of the
reference's serial fp32 sum bit for bit everywhere.

The file holds blur/<case>/{real, mac, mdim}, com/<case>, project/<dims>/m<mode>/s<scale>, project/const, lap/<dims>/<kind>,
curv/<dims>/<kind>/h<h> and the two loops: st/{iterations, phi, vel, curv} (scenes/surfaceTension.py) and dg/{iterations, com, density,
vel, xl_density, img_high, img_low} (the simMode 1 loop of manta_genSimData2.py with the constants of datagen_model.DG_LOOP).
"""
import ctypes
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen_model as M  # noqa: E402

f32 = np.float32


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def same(tag, got, want):
    assert M.same(got, want), "%s: the model differs from the reference (%d elements)" % (tag, M.differing(np.asarray(got), np.asarray(want)))


def record_blurs(call, out):
    for name, dims, sigma in M.blur_cases():
        sx, sy, sz = dims
        for ncomp, key in ((1, "real"), (3, "mac")):
            src = M.blur_input(name, ncomp)
            res = {}
            for inplace in (0, 1):
                dst = np.full(src.shape, M.SENTINEL, f32)
                after = np.full(src.shape, M.SENTINEL, f32)
                mdim = ctypes.c_int(-1)
                call("rec_blur", sx, sy, sz, ncomp, P(src), P(dst), fc(sigma), inplace, ctypes.byref(mdim), P(after))
                if not inplace:
                    same("blur/%s/%s: oG" % (name, key), after, src)
                res[inplace] = (dst, mdim.value)
            same("blur/%s/%s: oG is tG" % (name, key), res[1][0], res[0][0])
            want, wdim = M.blur(src, sigma)
            assert wdim == res[0][1] == res[1][1], (name, wdim, res[0][1])
            same("blur/%s/%s" % (name, key), want, res[0][0])
            out["blur/%s/%s" % (name, key)] = res[0][0]
            out["blur/%s/mdim" % name] = np.array([wdim], np.int32)
        print("blur", name, dims, sigma, "mDim", wdim)
    for q, (sigma, mdim) in enumerate(M.WEIGHT_SIGMAS):
        assert int(out["blur/w%d/mdim" % q][0]) == mdim, (sigma, mdim)
    special = out["blur/special/real"]
    assert np.isnan(special).any() and np.isfinite(special).any()


def record_com(call, out):
    for name in M.COM_CASES:
        d = M.com_input(name)
        sx, sy, sz = M.dims_of(d)
        c = np.full(3, M.SENTINEL, f32)
        call("rec_center_of_mass", sx, sy, sz, P(d), P(c))
        same("com/%s: the serial statement" % name, M.center_of_mass_serial(d), c)
        got = M.center_of_mass(d)
        if name in M.COM_EXACT:
            same("com/%s" % name, got, c)
        else:
            bound = M.com_bound(d, c)
            err = [abs(float(got[q]) - float(c[q])) for q in range(3)]
            assert all(e <= b for e, b in zip(err, bound)), (name, err, bound)
            print("com", name, "contract - reference", err, "bound", bound)
        out["com/%s" % name] = c
        print("com", name, c)


def record_projections(call, out):
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "p.ppm")

    def one(key, val, mode, scale):
        sx, sy, sz = M.dims_of(val)
        call("rec_project", sx, sy, sz, P(val), path.encode(), int(mode), fc(scale))
        img = M.read_ppm(path)
        want = M.project(val, mode, scale)
        assert open(path, "rb").read() == M.ppm_bytes(want), "%s: the file differs from the model's" % key
        same(key, want, img)
        out[key] = img

    for dims in M.PROJECT_DIMS:
        val = M.project_input(dims)
        for mode in M.PROJECT_MODES:
            for scale in M.PROJECT_SCALES:
                one(M.project_key(dims, mode, scale), val, mode, scale)
        print("projection", dims)
    one("project/const", M.project_const(), 1, 1.0)
    os.remove(path)
    os.rmdir(tmp)


def record_stencils(call, out):
    for key, kind, dims, h in M.stencil_cases():
        g = M.stencil_input(kind, dims)
        sx, sy, sz = dims
        res = np.full(g.shape, M.SENTINEL, f32)
        if h is None:
            call("rec_laplacian", sx, sy, sz, P(g), P(res))
            same(key, M.laplacian(g, np.full(g.shape, M.SENTINEL, f32)), res)
        else:
            call("rec_curvature", sx, sy, sz, P(g), P(res), fc(h))
            same(key, M.curvature(g, np.full(g.shape, M.SENTINEL, f32), h), res)
        assert (res == M.SENTINEL).any() and (res != M.SENTINEL).any()
        out[key] = res
    print("stencils done")


def record_loops(call, out):
    C = M.ST_LOOP
    n = C["res"] ** 3
    its = np.full(C["steps"], -9, np.int32)
    phi, vel, curv = np.zeros(n, f32), np.zeros(3 * n, f32), np.zeros(n, f32)
    call("rec_surface_tension", C["res"], C["steps"], P(its), P(phi), P(vel), P(curv))
    shape = (C["res"],) * 3
    out["st/iterations"], out["st/phi"], out["st/curv"] = its, phi.reshape(shape), curv.reshape(shape)
    out["st/vel"] = vel.reshape((3,) + shape)
    assert (its > 0).all() and np.abs(vel).max() > 0 and np.abs(curv).max() > 0
    print("surface tension loop: iterations", its, "max |vel|", np.abs(vel).max(), "max |curv|", np.abs(curv).max())

    C = M.DG_LOOP
    res, steps = C["res"], C["steps"]
    n, N = res ** 3, (2 * res) ** 3
    its = np.full((steps, 2), -9, np.int32)
    com = np.zeros((steps, 3), f32)
    dens, vel, xl = np.zeros(n, f32), np.zeros(3 * n, f32), np.zeros(N, f32)
    tmp = tempfile.mkdtemp()
    hi, lo = os.path.join(tmp, "high.ppm"), os.path.join(tmp, "low.ppm")
    A = lambda key, dt=f32: np.ascontiguousarray(np.array(C[key], dt))
    src, srcr, seeds, noise, ini, buoy = A("src"), A("srcr"), A("seeds", np.int32), A("noise"), A("ini"), A("buoy")
    call("rec_datagen_loop", res, steps, C["warm"], P(src), P(srcr), P(seeds), P(noise), P(ini), P(buoy), P(its), P(com), P(dens), P(vel), P(xl),
         hi.encode(), lo.encode())
    out["dg/iterations"], out["dg/com"] = its, com
    out["dg/density"], out["dg/vel"] = dens.reshape((res,) * 3), vel.reshape((3,) + (res,) * 3)
    out["dg/xl_density"] = xl.reshape((2 * res,) * 3)
    out["dg/img_high"], out["dg/img_low"] = M.read_ppm(hi), M.read_ppm(lo)
    same("dg/img_high", M.project(out["dg/xl_density"], 0, 5.0), out["dg/img_high"])
    same("dg/img_low", M.project(out["dg/density"], 0, 5.0), out["dg/img_low"])
    for f in (hi, lo):
        os.remove(f)
    os.rmdir(tmp)
    assert (its[:, 0] > 0).all() and (its[1::2, 1] > 0).all() and (its[0::2, 1] == -1).all()
    assert out["dg/img_high"].max() > 0 and out["dg/img_low"].max() > 0
    print("data-generation loop: iterations\n", its, "\ncentres\n", com, "\nmax density", dens.max(), xl.max(), "max |vel|", np.abs(vel).max())


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    record_blurs(call, out)
    record_com(call, out)
    record_projections(call, out)
    record_stencils(call, out)
    record_loops(call, out)
    path = M.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
