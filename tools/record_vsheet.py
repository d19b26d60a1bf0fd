"""Recorder of tests/golden/vsheet.npz: the reference's outputs for the cases of tests/vsheet_model.py (inputs are regenerated from its
seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything derived
from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the
reference checkout, B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/vortexplugins.cpp $B/plugin/vortexplugins.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libvsheet_rec.so $B/plugin/vortexplugins.cpp tools/vsheet_record.cpp \\
        -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_vsheet.py $B/libvsheet_rec.so

Before anything is written the recorder asserts that the numpy model reproduces every arithmetic array bit for bit, that the model's
smoothing weights are within vsheet_model.WEIGHT_ULPS of the reference's, that the reference's smoothVorticity output is reproduced
from the recorded table bit for bit (so the table is the one the plugin builds inside itself), and it refuses an input whose fp64 exp
is within one fp64 ulp of an fp32 rounding boundary (vsheet_model.weights_decided).

All texcoordInflow calls run in this one process in the order of vsheet_model.INFLOW_CALLS, first of all: the offset is a static of the
reference.  Keys: defaults/<channel>; calc/<mesh>/{vorticity, smokeAmount}; smoke/<mesh>/<shape>; source/<mesh>/<variant>/{vorticity};
smooth/<mesh>/<sigma>/{weights, index, out<iter>}; inflow/<call>/{t0, tex1, tex2}, inflow/reinit; loop/<step>/{...}.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_model as MM  # noqa: E402
import meshops_model as MO  # noqa: E402
import vsheet_model as M  # noqa: E402

f32, i32, i64 = np.float32, np.int32, ctypes.c_int64


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def C(a, dtype=f32):
    return np.ascontiguousarray(a, dtype)


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    assert got.tobytes() == want.tobytes(), "%s: the model differs from the reference in %d of %d entries" % (
        tag, int((got.view("u4") != want.view("u4")).sum()), got.size)


def shape_args(shape):
    if shape[0] == "box":
        return 0, P(C(shape[1])), P(C(shape[2]))
    return 1, P(C(shape[1])), P(C([shape[2]] * 3))


class Ref(object):
    def __init__(self, libpath):
        self.L = ctypes.CDLL(libpath)
        self.L.rec_last_error.restype = ctypes.c_char_p
        self.nt = self.nn = 0

    def call(self, name, *args):
        if getattr(self.L, name)(*args):
            raise RuntimeError(self.L.rec_last_error().decode())

    def open(self, m, dims, dt, opposite=None):
        self.nn, self.nt = m["pos"].shape[0], m["tris"].shape[0]
        self.call("rec_open", dims[0], dims[1], dims[2], fc(dt), i64(self.nn), P(C(m["pos"])), P(C(m["flags"], i32)), i64(self.nt), P(C(m["tris"], i32)),
                  None if opposite is None else P(C(opposite, i32)))

    def set(self, **ch):
        keep = {k: C(v) for k, v in ch.items()}
        self.call("rec_set", *[P(keep.get(k)) for k in ("vorticity", "vorticitySmoothed", "circulation", "smokeAmount", "smokeParticles")])

    def get(self):
        t, n = max(self.nt, 1), max(self.nn, 1)
        a = {"vorticity": np.zeros((t, 3), f32), "vorticitySmoothed": np.zeros((t, 3), f32), "circulation": np.zeros((t, 3), f32),
             "smokeAmount": np.zeros(t, f32), "smokeParticles": np.zeros(t, f32), "tex1": np.zeros((n, 3), f32), "tex2": np.zeros((n, 3), f32),
             "turb": np.zeros((n, 2), f32), "pos": np.zeros((n, 3), f32)}
        self.call("rec_get", *[P(a[k]) for k in ("vorticity", "vorticitySmoothed", "circulation", "smokeAmount", "smokeParticles", "tex1", "tex2",
                                                  "turb", "pos")])
        return {k: v[:(self.nt if k in M.DEFAULTS else self.nn)].copy() for k, v in a.items()}

    def offset(self):
        o = np.zeros(3, f32)
        self.call("rec_offset", P(o))
        return o

    def corners(self):
        o = np.zeros(max(3 * self.nt, 1), i32)
        self.call("rec_corners", P(o))
        return o[:3 * self.nt]

    def table(self, sigma):
        w, idx = np.zeros(max(3 * self.nt, 1), f32), np.zeros(max(3 * self.nt, 1), i32)
        self.call("rec_smooth_table", fc(sigma), P(w), P(idx))
        return w[:3 * self.nt], idx[:3 * self.nt]


def record_inflow(R, out):
    m = M.MESHES[M.INFLOW_MESH]()
    R.open(m, M.DIMS, M.DT)
    got = R.get()
    for k in M.DEFAULTS:                     # what clear(), addNode / addTri and rebuildChannels() leave: T() in every entry
        assert (got[k] == f32(M.DEFAULTS[k])).all(), k
        out["defaults/" + k] = got[k][:4]
    assert not got["tex1"].any() and not got["tex2"].any() and not got["turb"].any()
    out["defaults/tex1"], out["defaults/turb"] = got["tex1"][:4], got["turb"][:4]
    t0, tex1, tex2 = np.zeros(3, f32), got["tex1"], got["tex2"]
    for q, shape in enumerate(M.INFLOW_CALLS):
        vel = M.mac_grid("inflow%d" % q)
        R.call("rec_inflow", *(shape_args(shape) + (P(vel),)))
        got = R.get()
        t0, tex1, tex2 = M.texcoord_inflow(M.DIMS, vel, shape, M.DT, t0, m["pos"], tex1, tex2)
        same("inflow/%d/t0" % q, t0, R.offset())
        same("inflow/%d/tex1" % q, tex1, got["tex1"])
        same("inflow/%d/tex2" % q, tex2, got["tex2"])
        out["inflow/%d/t0" % q], out["inflow/%d/tex1" % q], out["inflow/%d/tex2" % q] = t0, got["tex1"], got["tex2"]
        print("inflow", q, "cells", len(M.inflow_cells(M.DIMS, shape)), "nodes inside", int(M.inside(shape, m["pos"]).sum()), "t0", t0)
        if q == 1:
            R.call("rec_reinit_tex")
            got = R.get()
            same("inflow/reinit", M.reinit_tex(m["pos"], t0), got["tex1"])
            same("inflow/reinit", got["tex1"], got["tex2"])
            out["inflow/reinit"] = got["tex1"]
            tex1 = tex2 = got["tex1"]
    assert np.isnan(t0).all() and len(M.inflow_cells(M.DIMS, M.INFLOW_CALLS[-1])) == 0          # cnt == 0 gives NaN


def record_stages(R, out):
    cnt = dict(small_area=0, clamped=0, fixed=0, zero_normal=0)
    for name, make in M.MESHES.items():
        m = M.with_fixed(make(), name)
        nt = m["tris"].shape[0]
        st = M.sheet_state(name, nt)
        R.open(m, M.DIMS, M.DT)
        # calcVorticity
        R.set(**st)
        R.call("rec_calc_vorticity")
        got = R.get()
        v, smoke = M.calc_vorticity(m, st["circulation"])
        same("calc/%s/vorticity" % name, v, got["vorticity"])
        same("calc/%s/smokeAmount" % name, smoke, got["smokeAmount"])
        out["calc/%s/vorticity" % name], out["calc/%s/smokeAmount" % name] = got["vorticity"], got["smokeAmount"]
        cnt["small_area"] += int((M.face_area(m).astype(np.float64) < 1e-10).sum())
        cnt["zero_normal"] += int((~M.face_normal(m).any(1)).sum()) if nt else 0
        # meshSmokeInflow
        for sname, shape in M.SMOKE_SHAPES.items():
            R.set(**st)
            R.call("rec_smoke_inflow", *(shape_args(shape) + (fc(0.37),)))
            got = R.get()
            same("smoke/%s/%s" % (name, sname), M.smoke_inflow(m, shape, 0.37, st["smokeAmount"]), got["smokeAmount"])
            out["smoke/%s/%s" % (name, sname)] = got["smokeAmount"]
        # vorticitySource
        vel, old = M.mac_grid("src-" + name), M.mac_grid("src-old-" + name)
        for vname, (with_vel, maxAmount, mult, scale) in M.SOURCE_VARIANTS.items():
            R.set(**st)
            R.call("rec_source", P(C(M.GRAVITY)), P(vel) if with_vel else None, P(old) if with_vel else None, fc(scale), fc(maxAmount), fc(mult))
            got = R.get()
            w, vn = M.vorticity_source(m, st["vorticity"], M.GRAVITY, M.DIMS, M.DT, vel if with_vel else None, old if with_vel else None, scale,
                                       maxAmount, mult)
            same("source/%s/%s" % (name, vname), w, got["vorticity"])
            out["source/%s/%s" % (name, vname)] = got["vorticity"]
            cnt["clamped"] += int(((maxAmount > 0) & (vn > f32(maxAmount))).sum())
        cnt["fixed"] += int(M.tri_fixed(m).sum())
        print("stages", name, nt, "triangles")
    print("stage counters:", cnt)
    assert all(v > 0 for v in cnt.values()), cnt


def record_smooth(R, out):
    worst, differing, total = 0, 0, 0
    for name, make in list(M.MESHES.items()) + list(M.OPEN_MESHES.items()):
        m = make()
        nt = m["tris"].shape[0]
        is_open = name in M.OPEN_MESHES
        opp = MO.corners(m["tris"])[0]
        st = M.sheet_state(name, nt)
        R.open(m, M.DIMS, M.DT, opp if is_open else None)
        if not is_open:
            assert np.array_equal(R.corners(), opp), name                 # the model's corner table is the reference's
        else:
            assert (opp < 0).any()
        for sigma in M.SMOOTH_SIGMAS:
            w_ref, idx_ref = R.table(sigma)
            arg, t, has = M.smooth_args(m, opp, sigma)
            assert M.weights_decided(arg[has]) == 0, "%s sigma %g: an exp is undecided within one fp64 ulp; choose another input" % (name, sigma)
            w, idx = M.smooth_weights(m, opp, sigma)
            assert np.array_equal(idx, idx_ref)
            d = M.ulps_apart(w, w_ref)
            assert d.max(initial=0) <= M.WEIGHT_ULPS, (name, sigma, int(d.max()))
            worst, differing, total = max(worst, int(d.max(initial=0))), differing + int((d != 0).sum()), total + d.size
            key = "smooth/%s/%g" % (name, sigma)
            out[key + "/weights"], out[key + "/index"] = w_ref, idx_ref
            for it in M.SMOOTH_ITERS:
                R.set(**st)
                R.call("rec_smooth", it, fc(sigma), fc(M.ALPHA))
                got = R.get()
                same(key + "/vorticity", st["vorticity"], got["vorticity"])
                _, sm = M.smooth_iterate(w_ref, idx_ref, st["vorticity"], it, M.ALPHA)
                same("%s/out%d" % (key, it), sm, got["vorticitySmoothed"])      # the recorded table is the plugin's, and line 158's indexing
                out["%s/out%d" % (key, it)] = got["vorticitySmoothed"]
        print("smooth", name, nt, "triangles")
    print("weights: %d of %d differ from the reference's float exp, at most %d ulp" % (differing, total, worst))
    out["smooth/weight_stats"] = np.array([differing, total, worst], np.int64)


def record_loop(R, out):
    C_ = M.LOOP
    m, flags = M.loop_inputs()
    dims, dt = C_["dims"], C_["dt"]
    R.open(m, dims, dt)
    opp = MO.corners(m["tris"])[0]
    assert np.array_equal(R.corners(), opp)
    pos = m["pos"].copy()
    st = M.default_sheet(m["tris"].shape[0])
    for step in range(C_["steps"]):
        cur = dict(m, pos=pos)
        vel, old = M.loop_velocities(step)
        R.call("rec_smoke_inflow", *(shape_args(C_["smoke"]) + (fc(C_["amount"]),)))
        st["smokeAmount"] = M.smoke_inflow(cur, C_["smoke"], C_["amount"], st["smokeAmount"])
        R.call("rec_source", P(C(C_["gravity"])), P(vel), P(old), fc(C_["scale"]), fc(C_["maxAmount"]), fc(C_["mult"]))
        st["vorticity"], _ = M.vorticity_source(cur, st["vorticity"], C_["gravity"], dims, dt, vel, old, C_["scale"], C_["maxAmount"], C_["mult"])
        w_ref, idx_ref = R.table(C_["sigma"])
        arg, _, has = M.smooth_args(cur, opp, C_["sigma"])
        assert M.weights_decided(arg[has]) == 0, "loop step %d: an exp is undecided" % step
        assert M.ulps_apart(M.smooth_weights(cur, opp, C_["sigma"])[0], w_ref).max() <= M.WEIGHT_ULPS
        R.call("rec_smooth", C_["iters"], fc(C_["sigma"]), fc(C_["alpha"]))
        st["vorticitySmoothed"] = M.smooth_iterate(w_ref, idx_ref, st["vorticity"], C_["iters"], C_["alpha"])[1]
        n = dims[0] * dims[1] * dims[2]
        vvort, vvel, vrhs, vits = np.zeros((3, n), f32), np.zeros((3, n), f32), np.zeros((3, n), f32), np.zeros(3, i32)
        R.call("rec_vic", fc(C_["vic_sigma"]), P(flags), 1, fc(1.5), fc(1e-3), fc(C_["vic_scale"]), 2, P(vvort), P(vvel), P(vrhs), P(vits))
        cur_sheet = dict(cur)
        mvort, _, vbound = M.spread(cur_sheet, st["vorticity"], flags, dims, C_["vic_sigma"], want_bound=True)
        assert (np.abs(vvort.T.astype(np.float64) - mvort).max(1) <= vbound).all(), "loop step %d: spreading outside the bound" % step
        out["loop/%d/vic_vort" % step], out["loop/%d/vic_vel" % step], out["loop/%d/vic_iterations" % step] = vvort, vvel, vits
        R.call("rec_advect", P(flags), P(vvel), 2)       # the model's advection is fed the reference's VIC velocity
        pos = np.ascontiguousarray(MM.advect_nodes(dims, vvel, np.ascontiguousarray(pos.T), m["flags"], dt, 2).T)
        R.call("rec_reinit_tex")
        got = R.get()
        for k in M.DEFAULTS:
            same("loop/%d/%s" % (step, k), st[k], got[k])
        same("loop/%d/pos" % step, pos, got["pos"])
        same("loop/%d/tex1" % step, M.reinit_tex(pos, (0, 0, 0)), got["tex1"])
        same("loop/%d/tex2" % step, got["tex1"], got["tex2"])
        for k in ("vorticity", "vorticitySmoothed", "smokeAmount", "pos", "tex1"):
            out["loop/%d/%s" % (step, k)] = got[k]
        out["loop/%d/weights" % step] = w_ref
    assert (m["flags"] & 1).any() and not (m["flags"] & 1).all()
    print("loop: %d triangles, %d steps" % (m["tris"].shape[0], C_["steps"]))


def record_vic(R, out):
    """the spreading of every case (vort), and for vsheet_model.VIC_SOLVES the whole plugin on a MAC and on a Vec3 velocity grid"""
    worst, differing, total = 0.0, 0, 0
    for name, (dims, sigma, T, rev) in M.vic_cases().items():
        m, vorticity = M.vic_soup(dims, T, 1, rev)
        flags = M.vic_flags(dims)
        assert not M.spread_undecided(m, flags, dims, sigma), "%s: a cos is undecided within one fp64 ulp; choose another input" % name
        n = dims[0] * dims[1] * dims[2]
        R.open(m, dims, M.DT, np.full(3 * T, -1, i32))       # no corner table is needed
        R.set(vorticity=vorticity)
        kinds = (("mac", 1), ("vec3", 0)) if name in M.VIC_SOLVES else (("mac", 1),)
        for kind, mac in kinds:
            vort, vel, rhs = np.zeros((3, n), f32), np.zeros((3, n), f32), np.zeros((3, n), f32)
            its = np.zeros(3, i32)
            R.call("rec_vic", fc(sigma), P(flags), mac, fc(M.VIC_SOLVE["cgMaxIterFac"]), fc(M.VIC_SOLVE["cgAccuracy"]), fc(M.VIC_SOLVE["scale"]), 2,
                   P(vort), P(vel), P(rhs), P(its))
            if name in M.VIC_SOLVES:
                out["vic/%s/%s/vel" % (name, kind)], out["vic/%s/%s/iterations" % (name, kind)] = vel, its
                if n < 1000:
                    out["vic/%s/%s/rhs" % (name, kind)] = rhs
                print("vic", name, kind, "iterations", its)
        model, wnorm, bound = M.spread(m, vorticity, flags, dims, sigma, want_bound=True)
        ref = np.ascontiguousarray(vort.T)
        err = np.abs(ref.astype(np.float64) - model).max(1)
        assert (err <= bound).all(), (name, float((err - bound).max()))
        assert not ref[bound == 0].any() and not model[bound == 0].any()       # where nothing lands the entry is exactly 0
        hit = bound > 0
        if hit.any():
            worst = max(worst, float((err[hit] / bound[hit]).max()))
        differing, total = differing + int((ref != model).any(1).sum()), total + int(hit.sum())
        out["vic/%s/vort" % name] = vort
        print("vic", name, "entries", int(hit.sum()), "not bit-identical", int((ref != model).any(1).sum()), "wnorm inf", int(np.isinf(wnorm).sum()))
    for bad in (0, 3):                                       # the reference asserts in setICPreconditioner: its own default fails
        try:
            R.call("rec_vic", fc(1.5), P(flags), 1, fc(1.5), fc(1e-3), fc(0.01), bad, P(vort), P(vel), P(rhs), P(its))
            raise AssertionError("precondition %d ran" % bad)
        except RuntimeError as e:
            assert "setICPreconditioner: Invalid method specified." in str(e), str(e)
            out["vic/precondition%d" % bad] = np.frombuffer(str(e).split("\n")[0].encode(), np.uint8)
    print("spreading: %d of %d entries not bit-identical to the reference, largest error %.3g of the bound" % (differing, total, worst))
    out["vic/stats"] = np.array([differing, total, worst], np.float64)


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    R = Ref(libpath)
    out = {}
    record_inflow(R, out)          # first: the static offset of the process starts at zero
    record_stages(R, out)
    record_smooth(R, out)
    record_loop(R, out)
    record_vic(R, out)
    R.call("rec_close")
    path = M.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
