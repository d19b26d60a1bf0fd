"""Recorder of tests/golden/fields.npz: the reference's outputs for the fixture cases of tests/fields_model.py (inputs are regenerated
from its seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.
Everything derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP
thread, all cases in one process (REF: the reference checkout, B: any scratch directory outside the tree):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    for f in fire waves; do oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/$f.cpp $B/plugin/$f.cpp; done
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$B -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libfields_rec.so tools/fields_record.cpp -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_fields.py $B/libfields_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Arrays of more than fields_model.FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha.  Before anything is
written the recorder asserts that the numpy model reproduces every recorded array bit for bit -- except `flame` and `heat`, where the
reference's powf(x, 0.5f) and the model's correctly rounded square root may differ in the last bit: there it asserts the bounds of
DESIGN.md section 15, stores the differing cells (<key>#diffidx, <key>#diffref) and their number per case (fire/<case>/powf_cells).
The conditions each case exists for are asserted here and again, from the model's counters, in tests/test_fields_model.py.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fields_model as M  # noqa: E402

f32 = np.float32


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def soa(g):
    """[z][y][x][3] -> [3][n]"""
    return np.ascontiguousarray(np.asarray(g, f32).reshape(-1, 3).T)


def aos(a, shape):
    return np.ascontiguousarray(a.reshape(3, -1).T.reshape(shape + (3,)))


def fc(x):
    return ctypes.c_float(float(x))


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    u = "u%d" % got.dtype.itemsize
    d = got.view(u) != want.view(u)
    assert not d.any(), "%s: the model differs from the reference in %d of %d words, first at %s (%r vs %r)" % (
        tag, int(d.sum()), d.size, np.argwhere(d)[0], got[tuple(np.argwhere(d)[0])], want[tuple(np.argwhere(d)[0])])


def record_fire(call, out):
    cnt = {}
    for case, (name, absent, par) in M.FIRE_CASES.items():
        sx, sy, sz = M.DIMS[name]
        g = M.fire_inputs(name)
        for k in absent:
            g[k] = None
        ref = {k: (None if v is None else v.copy()) for k, v in g.items()}
        pv = np.array([par["burningRate"], par["flameSmoke"], par["ignitionTemp"], par["maxTemp"]] + list(par["color"]), f32)
        call("rec_process_burn", sx, sy, sz, fc(M.FIRE_DT), *[P(ref[k]) for k in ("fuel", "density", "react", "red", "green", "blue", "heat")], P(pv))
        model, mflame = M.run_fire(case, cnt)
        ncell = 0
        for k, a in ref.items():
            if a is None:
                assert k not in model
                continue
            key = "fire/%s/%s" % (case, k)
            if k == "heat":
                n = M.put_near(out, key, a, model[k])
                bound = M.heat_bound(M.fire_flame(case), a, par["ignitionTemp"], par["maxTemp"])
                assert (np.abs(a.astype(np.float64) - model[k].astype(np.float64)) <= bound).all(), key
                ncell += n
            else:
                same(key, model[k], a)
                M.put(out, key, a)
        flame = M.prefill(name, "flame")
        call("rec_update_flame", sx, sy, sz, P(ref["react"]), P(flame))
        key = "fire/%s/flame" % case
        n = M.put_near(out, key, flame, mflame)
        assert (np.abs(flame.astype(np.float64) - mflame.astype(np.float64)) <= M.ulp(flame)).all(), key
        out["fire/%s/powf_cells" % case] = np.array([ncell, n, int(M.interior_mask(flame.shape).sum())], np.int64)   # heat, flame, interior
        b = ~M.interior_mask(flame.shape)
        assert np.array_equal(flame[b], M.prefill(name, "flame")[b]) and np.array_equal(ref["fuel"][b], g["fuel"][b])
        print("fire", case, "cells where powf differs from sqrtf: heat %d, flame %d of %d" % (ncell, n, int((~b).sum())))
    print("fire branch counts:", cnt)
    for key in ("fuel_le_eps", "fuel_ge_1", "fuel_clamped", "emit_le_eps", "emit_gt_eps", "density_above_1", "react_zero_heat_kept", "heat_written",
                "absent_red", "absent_green", "absent_blue", "absent_heat"):
        assert cnt.get(key, 0) > 0, key


def record_waves(call, out):
    for name in M.ALL:
        sx, sy, sz = M.DIMS[name]
        curv = M.prefill(name, "curv")
        v = M.secderiv_input(name)
        call("rec_sec_deriv", sx, sy, sz, P(v), P(curv))
        same("secderiv/" + name, M.sec_deriv_2d(v, M.prefill(name, "curv")), curv)
        M.put(out, "secderiv/" + name, curv)
        for kind in M.SUM_KINDS:
            h = M.sum_input(name, kind)
            ref, sm = h.copy(), ctypes.c_float(0)
            call("rec_sum_normalize", sx, sy, sz, P(ref), fc(M.SUM_TARGET), ctypes.byref(sm))
            key = "sum/%s/%s" % (name, kind)
            same(key + "/sum", np.array([M.total_sum(h)], f32), np.array([sm.value], f32))
            same(key + "/grid", M.normalize_sum_to(h, M.SUM_TARGET), ref)
            assert np.isfinite(ref).all() and sm.value != 0, key
            out[key + "/sum"] = np.array([sm.value], f32)
            M.put(out, key + "/grid", ref)
        for cn in (0, 1):
            I = M.wave_inputs(name)
            sh = I["ut"].shape
            A = [np.full(sh, 7, f32) for _ in range(5)]
            call("rec_wave_system", sx, sy, sz, fc(M.wave_s(M.WAVE_DT, M.WAVE_CSQR)), cn, P(I["flags"]), P(I["ut"]), P(I["utm1"]), *[P(a) for a in A])
            model = M.run_wave_system(name, bool(cn))
            for k, a in zip(("A0", "Ai", "Aj", "Ak", "rhs"), A):
                key = "wavesys/%s/%d/%s" % (name, cn, k)
                same(key, model[k], a)
                M.put(out, key, a)
    for name in M.CG_DIMS:
        for cn in (0, 1):
            I = M.cg_inputs(name)
            sx, sy, sz = I["dims"]
            ut, utm1, o, it = I["ut"].copy(), I["utm1"].copy(), np.full(I["ut"].shape, 5, f32), ctypes.c_int(0)
            call("rec_cg_solve_we", sx, sy, sz, fc(M.CG_DT), P(I["flags"]), P(ut), P(utm1), P(o), cn, fc(M.CG_CSQR), fc(1.5), fc(1e-5), ctypes.byref(it))
            key = "cgwe/%s/%d" % (name, cn)
            assert it.value > 8, (key, it.value)
            same(key + "/utm1", I["ut"], utm1)
            same(key + "/out", ut, o)
            out[key + "/iterations"] = np.array([it.value], np.int64)
            out[key + "/ut"] = ut
            print(key, "iterations", it.value)


def record_uv(call, out):
    for name in M.ALL:
        sx, sy, sz = M.DIMS[name]
        sh = M.shape_of(M.DIMS[name])
        for oname, off in M.UV_OFFSETS.items():
            uv = soa(M.uv_prefill(name))
            call("rec_reset_uv", sx, sy, sz, P(uv), P(None if off is None else np.array(off, f32)))
            key = "resetuv/%s/%s" % (name, oname)
            same(key, M.reset_uv(sh, off), aos(uv, sh))
            M.put(out, key, aos(uv, sh))
    cnt = {}
    ws, resets = [], []
    tiny = soa(np.full((1, 2, 2, 3), 9, f32))
    for n, step, i in M.UVW_SCALARS:
        uv, w = tiny.copy(), ctypes.c_float(0)
        call("rec_update_uv_weight", 2, 2, 1, fc(M.uv_time(step)), fc(M.UV_DT), fc(M.UV_RESET), i, n, P(uv), None, ctypes.byref(w))
        mw, mreset = M.uv_weight(M.uv_time(step), M.UV_DT, M.UV_RESET, i, n, cnt)
        reset = bool(uv[0, 1] != 9)
        same("uvw/%d/%d/%d" % (n, step, i), np.array([mw], f32), np.array([w.value], f32))
        assert reset == mreset, (n, step, i)
        ws.append(w.value)
        resets.append(reset)
    out["uvw/weights"] = np.array(ws, f32)
    out["uvw/resets"] = np.array(resets, np.int32)
    print("uv branch counts:", cnt)
    for key in ("total_le_eps", "reset", "ramp_down"):
        assert cnt.get(key, 0) > 0, key
    for case, (name, oname, n, step, i) in M.UVW_GRID_CASES.items():
        sx, sy, sz = M.DIMS[name]
        sh = M.shape_of(M.DIMS[name])
        off = M.UV_OFFSETS[oname]
        uv, w = soa(M.uv_prefill(name)), ctypes.c_float(0)
        call("rec_update_uv_weight", sx, sy, sz, fc(M.uv_time(step)), fc(M.UV_DT), fc(M.UV_RESET), i, n, P(uv), P(None if off is None else np.array(off, f32)),
             ctypes.byref(w))
        model = M.run_uvw_grid(case)
        same("uvwgrid/" + case, model, aos(uv, sh))
        assert M.get_uv_weight(model) == f32(w.value)
        M.put(out, "uvwgrid/" + case, aos(uv, sh))
        out["uvwgrid/%s/weight" % case] = np.array([w.value], f32)


def record_extrap(call, out):
    cnt = {}
    for case, (name, kind, vtype, dist, ff, ft) in M.EXTRAP_CASES.items():
        sx, sy, sz = M.DIMS[name]
        sh = M.shape_of(M.DIMS[name])
        flags, val, dist, ff, ft = M.extrap_inputs(case)
        c = {}
        model = M.run_extrap(case, c)
        if vtype == "vec":
            a = soa(val)
            call("rec_extrapolate", sx, sy, sz, P(flags), P(a), 2, dist, ff, ft)
            ref = aos(a, sh)
        else:
            ref = val.copy()
            call("rec_extrapolate", sx, sy, sz, P(flags), P(ref), {"real": 0, "int": 1, "flag": 3}[vtype], dist, ff, ft)
        key = "extrap/" + case
        same(key, model, ref)
        M.put(out, key, ref)
        changed = int((np.ascontiguousarray(ref).view(np.uint32) != np.ascontiguousarray(val).view(np.uint32)).sum())
        print(key, "words changed:", changed, c)
        if kind == "notarget" or dist == 0:
            assert changed == 0, key
        elif name != "g3":
            assert changed > 0, key
        if kind == "blob" and dist > 0:      # the block is deeper than the distance: the last pass still writes, the one after would too
            assert c.get("written_pass_%d" % dist, 0) > 0, key
        for k, v in c.items():
            cnt[k] = cnt.get(k, 0) + v
    assert cnt.get("both_flags", 0) > 0 and cnt.get("written_pass_6", 0) > 0, cnt


def record_vortex(call, out):
    for name in M.VORTEX_CASES:
        I = M.vortex_inputs(name)
        sx, sy, sz = I["dims"]
        sh = M.shape_of(I["dims"])
        v = soa(I["vel"])
        call("rec_vortex", sx, sy, sz, P(I["phiObs"]), P(v), P(np.array(I["center"], f32)), fc(I["radius"]))
        ref = aos(v, sh)
        touched = (ref[..., 0] != I["vel"][..., 0])
        assert touched.any() and not touched.all(), name          # cells on both sides of phiObs >= -1
        assert np.array_equal(ref[..., 2], I["vel"][..., 2])
        M.put(out, "vortex/" + name, ref)


def record_loops(call, out):
    """the four loops of tests/test_gpu_fields.py against the reference's classes; small enough to be kept in full"""
    i64 = ctypes.c_int64
    # (a) test_1030_waveeq.py
    C = M.WAVE_LOOP
    sx, sy, _ = C["dims"]
    h0 = M.wave_loop_h0()
    assert 12 <= h0.sum() < h0.size / 4
    mass, its = np.zeros(C["steps"], f32), np.zeros(C["steps"], np.int32)
    h, vel = np.zeros_like(h0), np.zeros_like(h0)
    call("rec_loop_wave", sx, sy, C["steps"], C["switch_at"], fc(C["dt"]), fc(C["cSqr"]), fc(M.wave_loop_vel_factor()), P(h0), P(mass), P(its), P(h), P(vel))
    print("loop/wave: mass", mass, "iterations", its)
    assert (its[:C["switch_at"] + 1] == -1).all() and (its[C["switch_at"] + 1:] > 0).all() and np.isfinite(h).all()
    out.update({"loop/wave/h0": h0, "loop/wave/mass": mass, "loop/wave/iterations": its.astype(np.int64), "loop/wave/h": h, "loop/wave/vel": vel})
    # (b) test_1020_uvs.py
    C = M.UV_LOOP
    sx, sy, _ = C["dims"]
    sh = M.shape_of(C["dims"])
    uv = np.zeros((C["uvs"], 3, sx * sy), f32)
    w = np.zeros((C["steps"], C["uvs"]), f32)
    call("rec_loop_uv", sx, sy, C["steps"], C["uvs"], fc(C["dt"]), fc(C["resetTime"]), P(soa(M.uv_loop_vel())), P(uv), P(w))
    for i in range(C["uvs"]):
        out["loop/uv/uv%d" % i] = aos(uv[i], sh)
    out["loop/uv/weights"] = w
    # resets occur during the loop (grids 1 and 2: 20 steps of 0.5 do not reach resetTime for grid 0)
    resets = [sum(M.uv_weight(M.uv_time(t), C["dt"], C["resetTime"], i, C["uvs"])[1] for t in range(C["steps"])) for i in range(C["uvs"])]
    print("loop/uv: resets per grid", resets, "last weights", w[-1])
    assert sum(resets) >= 2
    # (c) test_1040_secOrderBnd.py
    C = M.BND_LOOP
    n = C["res"] * C["res"]
    sh = (1, C["res"], C["res"])
    frac, vel, its = np.zeros((3, n), f32), np.zeros((3, n), f32), np.zeros(C["steps"], np.int32)
    call("rec_loop_bnd", C["res"], C["steps"], P(frac), P(vel), P(its))
    print("loop/bnd: iterations", its)
    assert (its > 0).all() and 0 < (frac > 0).sum() and ((frac > 0) & (frac < 1)).any()
    out.update({"loop/bnd/fractions": aos(frac, sh), "loop/bnd/vel": aos(vel, sh), "loop/bnd/iterations": its.astype(np.int64)})
    # (d) scenes/fire.py
    C = M.FIRE_LOOP
    n = C["res"] ** 3
    sh = (C["res"],) * 3
    mask, src = M.fire_loop_sources()
    dts, its, grids, cells = np.zeros(C["steps"], f32), np.zeros(C["steps"], np.int32), np.zeros((9, n), f32), np.zeros(2, np.int64)
    call("rec_loop_fire", C["res"], C["steps"], P(M.fire_loop_params()), P(mask), P(np.ascontiguousarray(np.stack(src))), P(dts), P(its), P(grids), P(cells))
    print("loop/fire: dt", dts, "iterations", its, "cells where powf differs from sqrtf (processBurn, updateFlame):", cells)
    assert (its > 0).all() and (dts > 0).all() and np.isfinite(grids).all()
    out["loop/fire/dts"], out["loop/fire/iterations"], out["loop/fire/powf_cells"] = dts, its.astype(np.int64), cells
    for q, k in enumerate(M.FIRE_LOOP_GRIDS):
        out["loop/fire/" + k] = grids[q].reshape(sh)
    for q, k in enumerate("xyz"):
        out["loop/fire/vel_" + k] = grids[6 + q].reshape(sh)


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    record_fire(call, out)
    record_waves(call, out)
    record_uv(call, out)
    record_extrap(call, out)
    record_vortex(call, out)
    record_loops(call, out)
    path = os.path.join(ROOT, "tests", "golden", "fields.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
