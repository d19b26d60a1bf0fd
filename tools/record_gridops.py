"""Recorder of tests/golden/gridops.npz: the reference's outputs for the cases of tests/gridops_model.py (inputs are regenerated from its
seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything
derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the
reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin                         # the legacy whitewater plugins are not in that library: expand their file
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/secondaryparticles.cpp $B/plugin/secondaryparticles.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libgridops_rec.so $B/plugin/secondaryparticles.cpp tools/gridops_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_gridops.py $B/libgridops_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Before anything is written the recorder asserts that the numpy model reproduces every recorded array bit for bit -- the three fp64
sums included, because with one thread the reference sums serially and so does the model.

Keys: those of gridops_model's *_cases(); norm/<dims>/<kind> is [fill][bnd][L1, L2]; norm/big/<kind> is [L1, L2] of the 129x127x64 grid;
emission/<dims>/<q>, reset/<dims>/<q>/{vel, <grid>}, macdata/<dims>/b<bnd>, r2v/<dims>, v2r/<dims>/{x, y, z}, resample/<dims>,
swap/<dims>/<c1c2c3>, avg/<dims>/<flags>, i2r/<dims>, noise/..., legacy/<dims>/r<radius>/t<types>/{ta, wc, ke, ratio, normals},
interp/<dims>/<real|vec|mac> (getInterpolated at gridops_model.interp_positions), npzsize/file (getNpzFileSize of a grid file: the
library of oracle/ref.mk is built with zlib, where the reference's guard is inverted and the answer is (0, 0, 0); recorded as it is).
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gridops_model as M  # noqa: E402

f32, i32 = np.float32, np.int32
KIND = {"real": 0, "int": 1, "vec": 2}


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def C(a):
    return None if a is None else np.ascontiguousarray(a).copy()


def same(tag, want, got):
    assert M.same(np.asarray(want), np.asarray(got)), "%s: the model differs from the reference (%d elements)" % (
        tag, M.differing(np.asarray(want), np.asarray(got)))


def opener(libpath):
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())
    return call


def norm_ref(call, a, bnd, l2):
    dims = (a.shape[2], a.shape[1], a.shape[0])
    r = ctypes.c_float()
    call("rec_norm", 1 if a.dtype == i32 else (2 if a.ndim == 4 else 0), l2, *dims, bnd, P(C(a)), ctypes.byref(r))
    return f32(r.value)


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    call = opener(libpath)
    out = {}

    for key, dims, odims, ax, kind in M.permute_cases():
        a = C(M.distinct(dims, kind))
        if odims is None:
            o = np.empty_like(a)
            call("rec_permute", KIND[kind], *dims, *ax, 0, 0, 0, 1, P(a), P(o))
        else:
            o = C(M.out_fill(odims, kind))
            call("rec_permute", KIND[kind], *dims, *ax, *odims, 0, P(a), P(o))
        same(key, M.permute_model(dims, odims, ax, kind), o)
        out[key] = o
    print("permutations done")

    for key, dims, kind in M.norm_cases():
        got = M.norm_table(dims, kind, lambda a, bnd, l2: norm_ref(call, a, bnd, l2))
        same(key, M.norm_table(dims, kind, M.norm), got)
        out[key] = got
    for kind in M.KINDS:
        a = M.norm_input(M.NORM_BIG, kind, "random")
        got = np.array([norm_ref(call, a, 0, l2) for l2 in (0, 1)], f32)
        same("norm/big/" + kind, np.array([M.norm(a, 0, l2) for l2 in (0, 1)], f32), got)
        out["norm/big/" + kind] = got
    print("norms done")

    for key, dims, kind, keep in M.join_cases():
        a, b = M.join_inputs(dims, kind)
        got = C(a)
        call("rec_join", KIND[kind], *dims, P(got), P(C(b)), keep)
        same(key, M.join(a, b, keep), got)
        out[key] = got

    for key, dims, reg, mac, add in M.force_cases():
        flags, vel, force, region = M.force_inputs(dims)
        got = C(vel)
        call("rec_force_field", *dims, P(C(flags)), P(got), P(C(force)), P(C(region)) if reg else None, add, mac)
        same(key, M.force_model(dims, reg, mac, add), got)
        out[key] = got
    for dims in M.FORCE_DIMS:
        flags, vel, force, _ = M.force_inputs(dims)
        got = C(vel)
        call("rec_initial_velocity", *dims, P(C(flags)), P(got), P(C(force)))
        key = "initvel/" + M.name_of(dims)
        same(key, M.add_force_if_lower(flags, vel, force), got)
        out[key] = got
    print("force fields done")

    for key, dims, which, dist, inside in M.extrap_cases():
        vel, phi = M.extrap_phi(dims, which, inside)
        got = C(vel)
        call("rec_extrapolate_vec3", *dims, P(got), P(C(phi)), dist, inside)
        same(key, M.extrapolate_vec3_simple(vel, phi, dist, bool(inside)), got)
        out[key] = got
    print("extrapolation done")

    for dims in M.SMALL_DIMS:
        g = M.name_of(dims)
        flags, target, source, tex = M.emission_inputs(dims)
        for q, (with_tex, absolute, type_) in enumerate(M.EMISSION_CASES):
            got = C(target)
            call("rec_emission", *dims, P(C(flags)), P(got), P(C(source)), P(C(tex)) if with_tex else None, int(absolute), type_)
            key = "emission/%s/%d" % (g, q)
            same(key, M.apply_emission(flags, target, source, tex if with_tex else None, absolute, type_), got)
            out[key] = got

        flags, vel, grids = M.reset_inputs(dims)
        for q, names in enumerate(M.RESET_CASES):
            given = {k: C(grids[k]) for k in names}
            gv = C(vel)
            ptrs = (ctypes.c_void_p * 7)(*[given[k].ctypes.data if k in given else None for k in M.RESET_NAMES])
            call("rec_reset_in_obstacle", *dims, P(C(flags)), P(gv), ptrs, fc(M.RESET_VALUE))
            wv, wg = M.reset_in_obstacle(flags, vel, {k: grids[k] for k in names}, M.RESET_VALUE)
            same("reset/%s/%d/vel" % (g, q), wv, gv)
            out["reset/%s/%d/vel" % (g, q)] = gv
            for k in names:
                same("reset/%s/%d/%s" % (g, q, k), wg[k], given[k])
                out["reset/%s/%d/%s" % (g, q, k)] = given[k]

        flags, source, target = M.random_flags(dims, "macdata"), M.vec(dims, "macsrc"), M.vec(dims, "mactgt")
        for bnd in M.MAC_BNDS:
            got = C(target)
            call("rec_copy_mac_data", *dims, P(C(source)), P(got), P(C(flags)), M.MAC_FLAG, bnd)
            same("macdata/%s/b%d" % (g, bnd), M.copy_mac_data(source, target, flags, M.MAC_FLAG, bnd), got)
            out["macdata/%s/b%d" % (g, bnd)] = got

        x, y, z, v = M.real(dims, "x"), M.real(dims, "y"), M.real(dims, "z"), M.vec(dims, "v")
        got = C(v)
        call("rec_real_to_vec3", *dims, P(C(x)), P(C(y)), P(C(z)), P(got))
        same("r2v/" + g, np.stack([x, y, z], axis=3), got)
        out["r2v/" + g] = got
        gx, gy, gz = C(x), C(y), C(z)
        call("rec_vec3_to_real", *dims, P(C(v)), P(gx), P(gy), P(gz))
        for k, got, c in (("x", gx, 0), ("y", gy, 1), ("z", gz, 2)):
            same("v2r/%s/%s" % (g, k), np.ascontiguousarray(v[..., c]), got)
            out["v2r/%s/%s" % (g, k)] = got

        src, tgt = M.vec(dims, "macsrc"), M.vec(dims, "mactgt")
        got = C(tgt)
        call("rec_resample_mac_to_vec3", *dims, P(C(src)), P(got))
        same("resample/" + g, M.resample_mac_to_vec3(src, tgt), got)
        out["resample/" + g] = got

        for c in M.SWAPS:
            got = C(v)
            call("rec_swap_components", *dims, P(got), *c)
            key = "swap/%s/%d%d%d" % ((g,) + c)
            same(key, M.swap_components(v, *c), got)
            out[key] = got

        for which in M.AVG_FLAGS:
            fl = M.avg_flags(dims, which)
            r = ctypes.c_float()
            call("rec_grid_avg", *dims, P(C(x)), P(C(fl)), ctypes.byref(r))
            got = np.array([r.value], f32)
            same("avg/%s/%s" % (g, which), np.array([M.grid_avg(x, fl)], f32), got)
            out["avg/%s/%s" % (g, which)] = got

        src = M.int_input(dims)
        got = C(x)
        call("rec_int_to_real", *dims, P(C(src)), P(got), fc(M.INT_FACTOR))
        same("i2r/" + g, M.int_to_real(src, M.INT_FACTOR), got)
        out["i2r/" + g] = got
        print("small plugins", g, "done")

    # the model's tile and parameters come from the package on the CPU checker backend (tests/util.py builds it)
    import util
    from mantaflow_amd import _lib
    _lib.use_library(util.build_oracle(), "cpu")
    for key, dims, is_vec, w, nset in M.noise_cases():
        flags, target, weight = M.noise_inputs(dims, is_vec)
        got = C(target)
        call("rec_simple_noise", is_vec, *dims, P(C(flags)), P(got), P(C(weight)) if w else None, fc(M.NOISE_SCALE), nset)
        tile, params = M.noise_tile_and_params(dims, nset)
        same(key, M.apply_simple_noise(flags, target, tile, params, M.NOISE_SCALE, weight if w else None), got)
        assert not M.same(got, target)
        out[key] = got
    print("simple noise done")

    for key, dims, radius, t in M.legacy_cases():
        flags, vel, nrm, phi = M.legacy_inputs(dims, radius)
        itype, jtype = M.LEGACY_TYPES[t]
        assert M.legacy_preconditions(flags, radius, itype, jtype)
        f, v = C(flags), C(vel)
        for which, name, normal in ((0, "ta", None), (1, "wc", nrm)):
            tmin, tmax = M.LEGACY_TAU[name][t]
            got = np.full(flags.shape, np.nan, f32)
            call("rec_legacy", which, *dims, P(got), P(f), P(v), P(C(normal)), None, radius, fc(tmin), fc(tmax), fc(M.LEGACY_SCALE), itype, jtype)
            same("%s/%s" % (key, name), M.legacy_gather(which, flags, vel, normal, radius, tmin, tmax, M.LEGACY_SCALE, itype, jtype)[0], got)
            out["%s/%s" % (key, name)] = got
        tmin, tmax = M.LEGACY_TAU["ke"][t]
        got = np.full(flags.shape, np.nan, f32)
        call("rec_legacy", 2, *dims, P(got), P(f), P(v), None, None, 0, fc(tmin), fc(tmax), fc(M.LEGACY_SCALE), itype, 0)
        same(key + "/ke", M.legacy_kinetic(flags, vel, tmin, tmax, M.LEGACY_SCALE, itype), got)
        out[key + "/ke"] = got
        itype, jtype = M.LEGACY_RATIO_TYPES[t]
        assert M.legacy_preconditions(flags, radius, itype, jtype, with_centres=False)
        got = np.full(flags.shape, np.nan, f32)
        call("rec_legacy", 3, *dims, P(got), P(f), None, None, None, radius, fc(0), fc(0), fc(0), itype, jtype)
        same(key + "/ratio", M.legacy_ratio(flags, radius, itype, jtype), got)
        walled = got[dims[2] // 2 if dims[2] > 1 else 0, dims[1] // 2, dims[0] // 2]
        # the walled-in cell: 0 / 0 in 3-D; in 2-D it meets itself on the aliased planes z != k, 2 radius times, and they all count
        assert np.isnan(walled) if dims[2] > 1 else walled == 1, (key, walled)
        assert t == 1 or ((got > 0) & (got < 1)).any(), key
        out[key + "/ratio"] = got
        if t == 0:
            got = C(nrm)
            call("rec_legacy", 4, *dims, None, None, None, P(got), P(C(phi)), 0, fc(0), fc(0), fc(0), 0, 0)
            same(key + "/normals", M.surface_normals(nrm, phi), got)
            out[key + "/normals"] = got
    print("legacy potentials done")

    for key, dims, kind in M.interp_cases():
        a, pos = M.interp_input(dims, kind), M.interp_positions(dims)
        got = np.zeros((len(pos), 3), f32)
        call("rec_interpolated", {"real": 0, "vec": 2, "mac": 3}[kind], *dims, P(C(a)), len(pos), P(C(pos)), P(got))
        got = C(got[:, 0]) if kind == "real" else got
        same(key, M.interpolate(a, pos, kind == "mac"), got)
        out[key] = got
    print("getInterpolated done")

    # getNpzFileSize of a grid file as Grid.save writes it (arr_0 is [z][y][x]), and of a name that does not exist
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, "g.npz")
        np.savez_compressed(name, arr_0=M.real(M.NPZ_DIMS, "npz"))
        got = np.zeros(3, f32)
        call("rec_npz_file_size", name.encode(), P(got))
        out["npzsize/file"] = got
        print("getNpzFileSize of a %s grid file:" % (M.NPZ_DIMS,), got)
    print("getNpzFileSize done")

    np.savez_compressed(M.GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (M.GOLDEN, len(out), os.path.getsize(M.GOLDEN)))
    assert os.path.getsize(M.GOLDEN) < 1000000


if __name__ == "__main__":
    main(sys.argv[1])
