"""Recorder of tests/golden/grid4d.npz and tests/golden/grid4d_vec4.uni: the reference's outputs for the cases of tests/grid4d_model.py
(inputs are regenerated from its seeded generators, never stored).  No test runs this; it needs the reference checkout and the build of
oracle/ref.mk.  Everything derived from the reference's text stays in a scratch directory outside the tree.  Run on the CPU machine
with one OpenMP thread, all cases in one process (REF: the reference checkout, B: any scratch directory outside the tree):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libgrid4d_rec.so tools/grid4d_record.cpp -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_grid4d.py $B/libgrid4d_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Arrays of more than grid4d_model.FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha.  Before anything is
written the recorder asserts that the numpy model reproduces every recorded array and scalar bit for bit, and that the model's branch
counters saw every branch the cases exist for.  The loops of test_2005_symmAdv.py and test_2065_partIo.py have no model: they are
runs of the reference's classes, kept for the GPU test to compare with.  The reference's messages (first line of the exception) are recorded as strings.
"""
import ctypes
import gzip
import os
import struct
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid4d_model as M  # noqa: E402

f32 = np.float32
KIND = {k: q for q, k in enumerate(M.KINDS)}
OPS = {k: q for q, k in enumerate(M.ELEMENTWISE + M.REDUCTIONS + ("setBound", "setBoundNeumann"))}
UNI_HEADER = "<6i252siQ"


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    u = "u%d" % got.dtype.itemsize
    d = got.view(u) != want.view(u)
    assert not d.any(), "%s: the model differs from the reference in %d of %d words, first at %s (%r vs %r)" % (
        tag, int(d.sum()), d.size, np.argwhere(d)[0], got[tuple(np.argwhere(d)[0])], want[tuple(np.argwhere(d)[0])])


def params(kind, op):
    if op in ("setConst", "addConst", "multConst", "setBound"):
        v = M.CONST[kind]
    elif op == "addScaled":
        v = M.FACTOR[kind]
    elif op == "clamp":
        v = M.CLAMP[kind]
    else:
        v = 0
    p = np.zeros(4, f32)
    v = np.atleast_1d(np.array(v, f32))
    p[:v.size] = v
    return p


def record_ops(call, out):
    cnt = {}
    for key, name, dims, kind, op, arg in M.op_cases():
        a, b = M.rand_grid(dims, kind, "a"), M.rand_grid(dims, kind, "b")
        ref, sc = a.copy(), ctypes.c_float(0)
        call("rec_g4_op", KIND[kind], OPS[op], *dims, P(ref), P(b), P(params(kind, op)), 0 if arg is None else arg, ctypes.byref(sc))
        model = M.run_op(dims, kind, op, arg, cnt)
        if op in M.REDUCTIONS:
            same(key, model, np.array([sc.value], f32))
            same(key + " (input)", ref, a)
            out[key] = model
        else:
            same(key, model, ref)
            M.put(out, key, ref)
    print("op branch counts:", cnt)
    assert cnt["bound_cells"] > 0 and cnt["inner_cells"] > 0 and all(cnt["neumann_axes_%d" % n] > 0 for n in range(5)), cnt


def record_small(call, out):
    cnt = {}
    dims = M.SHAPES["a"]
    for rname, (start, end) in M.REGIONS.items():
        for kind in ("real", "vec4"):
            a = M.rand_grid(dims, kind, "a")
            ref = a.copy()
            val = np.zeros(4, f32)
            v = np.atleast_1d(np.array(M.REGION_VALUE[kind], f32))
            val[:v.size] = v
            call("rec_g4_region", int(kind == "vec4"), *dims, P(ref), P(np.array(start, f32)), P(np.array(end, f32)), P(val))
            key = "region/%s/%s" % (rname, kind)
            c = {}
            same(key, M.set_region(a, dims, start, end, M.REGION_VALUE[kind], c), ref)
            cnt["region_" + rname] = c["region_cells"]
            M.put(out, key, ref)
    assert cnt["region_none"] == 0 and cnt["region_all"] == np.prod(dims) and 0 < cnt["region_frac"] < cnt["region_all"], cnt
    for sname, (shape, srct, ddims) in M.SLICES.items():
        sd = M.SHAPES[shape]
        for kind in ("real", "vec4"):
            src = M.rand_grid(sd, kind, "a")
            r = np.random.default_rng(M._seed("slice", sname, kind))
            dsh = (ddims[2], ddims[1], ddims[0])
            dst = r.uniform(-9, 9, dsh + ((3,) if kind == "vec4" else ())).astype(f32)
            dstt = r.uniform(-9, 9, dsh).astype(f32) if kind == "vec4" else None
            for with_t in ((False, True) if kind == "vec4" else (False,)):
                rd, rt = dst.copy(), (dstt.copy() if with_t else None)
                call("rec_g4_slice", int(kind == "vec4"), *sd, P(src), srct, *ddims, P(rd), P(rt))
                md, mt = M.get_slice(src, srct, dst, dstt if with_t else None, cnt)
                key = "slice/%s/%s%s" % (sname, kind, "/t" if with_t else "")
                same(key, md, rd)
                M.put(out, key, rd)
                if with_t:
                    same(key + "/dstt", mt, rt)
                    M.put(out, key + "/dstt", rt)
    assert cnt.get("slice_out_of_range", 0) > 0 and cnt.get("slice_smaller_dst", 0) > 0, cnt
    for shape in ("a", "c"):
        sd = M.SHAPES[shape]
        for c in range(4):
            v, r = M.rand_grid(sd, "vec4", "a"), M.rand_grid(sd, "real", "b")
            rv, rr = v.copy(), r.copy()
            call("rec_g4_comp", 0, *sd, P(rv), P(rr), c)
            same("getComp/%s/%d" % (shape, c), M.get_comp(v, c), rr)
            same("getComp/%s/%d (src)" % (shape, c), v, rv)
            M.put(out, "getComp/%s/%d" % (shape, c), rr)
            rv, rr = v.copy(), r.copy()
            call("rec_g4_comp", 1, *sd, P(rv), P(rr), c)
            same("setComp/%s/%d" % (shape, c), M.set_comp(r, v, c), rv)
            M.put(out, "setComp/%s/%d" % (shape, c), rv)


def osz(kw):
    return np.array(list(kw.get("offset", (0,) * 4)) + list(kw.get("scale", (1,) * 4)) + list(kw.get("size", (-1,) * 4)), f32)


def record_interp(call, out):
    cnt = {}
    for kind in ("real", "vec4"):
        src = M.rand_grid(M.INTERP_CHAIN[0][1], kind, "chain")
        for name, sd, td in M.INTERP_CHAIN:
            ref = M.garbage(td, kind)
            call("rec_g4_interp", int(kind == "vec4"), *td, P(ref), *sd, P(src), P(osz({})))
            key = "interp/%s/%s" % (name, kind)
            same(key, M.interpolate(src, td, cnt=cnt), ref)
            M.put(out, key, ref)
            src = ref
        for name, (sd, td, kw) in M.INTERP_CASES.items():
            src = M.rand_grid(sd, kind, "interp")
            ref = M.garbage(td, kind)
            call("rec_g4_interp", int(kind == "vec4"), *td, P(ref), *sd, P(src), P(osz(kw)))
            key = "interp/%s/%s" % (name, kind)
            same(key, M.interpolate(src, td, cnt=cnt, **kw), ref)
            assert np.isfinite(ref).all(), key
            M.put(out, key, ref)
    print("interpolation branch counts:", cnt)
    for ax in "xyzt":
        for b in ("lower", "upper", "centre"):
            assert cnt.get("interp_%s_%s" % (b, ax), 0) > 0, (b, ax)


def first_line(call, *args):
    try:
        call(*args)
    except RuntimeError as e:
        return str(e).split("\n")[0]
    raise AssertionError("the reference accepted %r" % (args,))


def record_scripts(call, out):
    """the two harness sequences as runs of the reference's own classes, step by step through the same entries"""
    dims = (3, 3, 3, 3)
    want = M.script32_model()
    for kind, (c1, c2, add, mul, half) in M.SCRIPT32.items():
        dt = np.int32 if kind == "int" else f32
        nc = M.NCOMP[kind]

        def op(name, a, b, v):
            p = np.zeros(4, f32)
            p[:nc] = v
            a = a.copy()
            call("rec_g4_op", KIND[kind], OPS[name], *dims, P(a), P(b), P(p), 0, ctypes.byref(ctypes.c_float(0)))
            return a
        z = np.zeros(M.shape_of(dims, kind), dt)
        g1 = op("addConst", op("setConst", z, z, c1), z, add)
        g2 = op("multConst", op("setConst", z, z, c2), z, mul)
        g3 = op("addScaled", op("add", g1, g2, 0), g2, half)          # copyFrom(g1), add(g2), addScaled(g2, half)
        for q, g in enumerate((g1, g2, g3)):
            assert (g == g.flat[0]).all()
        got = np.array([g1.flat[0], g2.flat[0], g3.flat[0]], dt)
        same("script32/" + kind, want[kind], got)
        out["script32/" + kind] = got
    print("script32:", {k: v.tolist() for k, v in want.items()})
    want = M.script42_model()
    sm, nm, xl = (M.SCRIPT42_RES // 2,) * 4, (M.SCRIPT42_RES,) * 4, (M.SCRIPT42_RES * 2,) * 4
    rs, re = f32(sm[0] * 0.3), f32(sm[0] * 0.7)
    for kind, tag in (("real", "density"), ("vec4", "v3")):
        vec = int(kind == "vec4")
        g = {}
        g["sm_" + tag] = np.zeros(M.shape_of(sm, kind), f32)
        call("rec_g4_region", vec, *sm, P(g["sm_" + tag]), P(np.full(4, rs, f32)), P(np.full(4, re, f32)), P(np.ones(4, f32)))
        for dst, src, td, sd in ((tag, "sm_" + tag, nm, sm), ("xl_" + tag, tag, xl, nm), (tag + "2", "xl_" + tag, nm, xl), ("sm_" + tag + "2", tag + "2", sm, nm)):
            g[dst] = M.garbage(td, kind)
            call("rec_g4_interp", vec, *td, P(g[dst]), *sd, P(g[src]), P(osz({})))
        for name, dims in ((tag, nm), (tag + "2", nm), ("sm_" + tag, sm), ("sm_" + tag + "2", sm), ("xl_" + tag, xl)):
            d = np.zeros((dims[2], dims[1], dims[0]) + ((3,) if vec else ()), f32)
            call("rec_g4_slice", vec, *dims, P(g[name]), int(dims[0] * 0.5), *dims[:3], P(d), None)
            g["slice_" + name] = d
        for k, a in g.items():
            same("script42/" + k, want[k], a)
            M.put(out, "script42/" + k, a)
        assert 0 < g["sm_" + tag].sum() < g["sm_" + tag].size and np.isfinite(g["sm_" + tag + "2"]).all()


PD_KIND = {"real": 0, "int": 1, "vec3": 2}
PD_OPS = {k: q for q, k in enumerate(("add", "sub", "mult", "safeDiv", "addConst", "addScaled", "multConst", "clamp", "clampMin", "clampMax", "setConstRange",
                                      "setConstIntFlag", "getMin", "getMax", "getMaxAbs", "sum", "sumFlag", "sumSquare", "sumMagnitude"))}
PD_FILE_N = 37


def record_pdata(call, out):
    """every particle-data method; the sums are the reference's one-thread fp32 sums, kept beside nothing else: the package's contract is
    checked against them with the bound of tests/grid4d_model.py, which the reference itself must meet here"""
    worst = 0.0
    for key, n, kind, op in M.pd_cases():
        a, b, t = M.pd_inputs(key, n, kind, op)
        what = op.split("/")[0]
        par = np.zeros(4, f32)
        v = M.PD_FACTOR[kind] if what == "addScaled" else M.PD_CLAMP[kind] if what == "clamp" else M.PD_CONST[kind]
        if what == "clampMin":
            v = M.PD_CLAMP[kind][0]
        if what == "clampMax":
            v = M.PD_CLAMP[kind][1]
        v = np.atleast_1d(np.array(v, f32))
        par[:v.size] = v
        code = PD_OPS["sumFlag" if (what == "sum" and t is not None) else what]
        ref, res = a.copy(), np.zeros(3, f32)
        rng = M.pd_range(n)
        call("rec_pd_op", PD_KIND[kind], code, n, P(ref), P(b), P(t), P(par), M.PD_FLAG if t is not None else rng[0], rng[1], P(res))
        if op in M.PD_ARRAY_OPS:
            same(key, M.pd_array_op(kind, op, a, b, t), ref)
            M.put(out, key, ref)
        elif op in M.PD_MINMAX:
            same(key, np.array([M.pd_min_max(kind, op, a)], f32), res[:1])
            out[key] = res[:1].copy()
        else:
            terms = M.pd_terms(kind, op, a, t)
            model = M.pd_sum_reference(terms)
            got = res.view(np.int32)[:1].copy() if model.dtype == np.int32 else res[:model.size].copy()
            same(key, model, got)
            out[key] = got
            if model.dtype != np.int32:
                exact, bound = M.pd_sum_bound(terms)
                err = np.abs(got.astype(np.float64) - exact)
                assert (err <= bound).all(), (key, err, bound)
                if key.startswith("pdx/"):
                    assert (err == 0).all(), key
                elif bound.max() > 0:
                    worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    print("pdata sums: the reference's largest error as a share of the bound: %.4f" % worst)
    golden = os.path.join(ROOT, "tests", "golden")
    cwd = os.getcwd()
    msg = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for kind in M.PD_KINDS:
                a = M.pd_rand(PD_FILE_N, kind, "file")
                for ext in ("uni", "raw"):
                    name = "p_%s.%s" % (kind, ext)
                    call("rec_pd_file", PD_KIND[kind], 1, PD_FILE_N, P(a.copy()), name.encode())
                    raw = gzip.open(name, "rb").read()
                    assert raw[:4] == b"PD01"
                    h = struct.unpack("<6i256sQ", raw[4:4 + 288])
                    out["pdfile/%s/header" % kind] = np.array(h[:6], np.int64)       # count, solver dims, elementType, bytesPerElement
                    assert raw[4 + 288:] == a.tobytes(), (kind, ext)
                    back = np.zeros_like(a)
                    call("rec_pd_file", PD_KIND[kind], 0, PD_FILE_N, P(back), name.encode())
                    same("pdfile/%s/%s" % (kind, ext), back, a)
            with open("p_vec3.uni", "rb") as f:
                blob = f.read()
            with open(os.path.join(golden, "grid4d_pdata_vec3.uni"), "wb") as f:
                f.write(blob)
            z = np.zeros(PD_FILE_N, f32)
            msg["pd_save_noext"] = first_line(call, "rec_pd_file", 0, 1, PD_FILE_N, P(z), b"noext")
            msg["pd_save_unknown"] = first_line(call, "rec_pd_file", 0, 1, PD_FILE_N, P(z), b"p.foo")
            msg["pd_load_noext"] = first_line(call, "rec_pd_file", 0, 0, PD_FILE_N, P(z), b"noext")
            msg["pd_load_unknown"] = first_line(call, "rec_pd_file", 0, 0, PD_FILE_N, P(z), b"p.foo")
            msg["pd_load_type"] = first_line(call, "rec_pd_file", 0, 0, PD_FILE_N, P(z), b"p_vec3.uni")
        finally:
            os.chdir(cwd)
    for k, v in msg.items():
        print("message", k, "=", repr(v))
        out["message/" + k] = np.array(v)


def record_harness(call, out):
    """checkSymmetry / checkSymmetryVec3, testInitGridWithPos, setNoisePdata*, addTestParts"""
    cnt, digests = {}, {}
    for shape, axis, sym, bound in M.SYM_CASES:
        dims = M.SYM_SHAPES[shape]
        for vec in (False, True):
            for dis in (M.SYM_DISABLE if vec else (0,)):
                for with_err in (True, False):
                    a = M.sym_input(shape, vec)
                    ra = a.copy()
                    re = (np.zeros(a.shape[:3], f32) if vec else np.full(a.shape, np.nan, f32)) if with_err else None
                    if vec and with_err:
                        re[:] = 7          # err->setConst(0) comes first
                    call("rec_symmetry", int(vec), *dims, P(ra), P(re), int(sym), axis, bound, dis)
                    ma, me = M.check_symmetry(dims, a, with_err, sym, axis, bound, dis, cnt=cnt)
                    la, le = M.check_symmetry(dims, a, with_err, sym, axis, bound, dis, literal=True)
                    key = M.sym_key(shape, axis, sym, bound, vec, dis, with_err)
                    same(key, ma, ra)
                    same(key + " (literal)", la, ra)
                    digests[key] = M.sha(ra)
                    if with_err:
                        same(key + "/err", me, re)
                        same(key + "/err (literal)", le, re)
                        digests[key + "/err"] = M.sha(re)
    out["symsha/keys"], out["symsha/shas"] = np.array(list(digests.keys())), np.array(list(digests.values()))
    print("symmetry branch counts:", cnt)
    assert all(cnt.get(k, 0) > 0 for k in ("sym_pass0", "sym_pass1", "sym_centre", "sym_skipped")), cnt
    for shape, dims in M.SYM_SHAPES.items():
        g = np.full((dims[2], dims[1], dims[0]), np.nan, f32)
        call("rec_init_pos", *dims, P(g))
        same("initpos/" + shape, M.init_grid_with_pos(dims), g)
        M.put(out, "initpos/" + shape, g)
    for kind, (c1, c2, add, mul, half) in M.SCRIPT32.items():        # test_0500_pdataop.py: the same arithmetic on channels of ten slots
        if kind == "vec4":
            continue
        dt = np.int32 if kind == "int" else f32
        nc = 3 if kind == "vec3" else 1

        def pop(name, a, b, v):
            p = np.zeros(4, f32)
            p[:nc] = v
            a = a.copy()
            call("rec_pd_op", PD_KIND[kind], PD_OPS[name], 10, P(a), P(b), None, P(p), 0, 0, P(np.zeros(3, f32)))
            return a
        z = np.zeros((10, 3) if nc == 3 else (10,), dt)
        g1 = pop("addConst", np.full_like(z, c1), z, add)
        g2 = pop("multConst", np.full_like(z, c2), z, mul)
        g3 = pop("addScaled", pop("add", g1, g2, 0), g2, half)
        got = np.array([g1.flat[0], g2.flat[0], g3.flat[0]], dt)
        assert all((g == g.flat[0]).all() for g in (g1, g2, g3))
        same("script500/" + kind, M.script32_model()[kind], got)
        out["script500/" + kind] = got
    pos = M.noise_positions()
    for kind, q, dt, shape in (("real", 0, f32, (M.NOISE_N,)), ("int", 1, np.int32, (M.NOISE_N,)), ("vec3", 2, f32, (M.NOISE_N, 3))):
        o = np.zeros(shape, dt)
        call("rec_pd_noise", q, *M.NOISE_DIMS, 265, M.NOISE_N, P(pos), P(o), ctypes.c_float(M.NOISE_SCALE[kind]))
        assert np.isfinite(o.astype(np.float64)).all() and len(np.unique(o)) > 10, (kind, np.unique(o)[:20])
        M.put(out, "noise/" + kind, o)
    for case in M.ADDPARTS:
        I = M.addparts_inputs(case)
        n = I["n0"] + I["num"]
        buf = {k: np.concatenate([I[k], np.zeros((I["num"],) + I[k].shape[1:], I[k].dtype)]) for k in ("pos", "flags", "real", "vec", "ints", "plain")}
        size = ctypes.c_int(0)
        call("rec_add_test_parts", *M.ADDPARTS_DIMS, I["n0"], I["num"], *[P(buf[k]) for k in ("pos", "flags", "real", "vec", "ints", "plain")],
             P(I["src_real"]), P(I["src_mac"]), ctypes.byref(size))
        assert size.value == n, (case, size.value, n)
        want = M.add_test_parts(I)
        for k in buf:
            same("addparts/%s/%s" % (case, k), want[k], buf[k])
            out["addparts/%s/%s" % (case, k)] = buf[k]


def record_loops(call, out):
    """the loops of test_2005_symmAdv.py (res 12, 2 steps per field, 2-D and 3-D, every direction) and test_2065_partIo.py (res 16) as
    runs of the reference's own classes.  2-D arrays are kept in full; of a 3-D run the final phi and the final error grids are kept in
    full and the other grids as their largest magnitude and fp64 sum of magnitudes"""
    res, steps = M.LOOP2005["res"], M.LOOP2005["steps"]
    for dim in (2, 3):
        sh = (res if dim == 3 else 1, res, res)
        n = int(np.prod(sh))
        for symms in range(2 * dim):
            ps, vs, phi, vel = np.zeros(sh, f32), np.zeros(sh + (3,), f32), np.zeros(sh, f32), np.zeros(sh + (3,), f32)
            errs, first, it = np.zeros((4,) + sh, f32), np.zeros(2, f32), ctypes.c_int(0)
            call("rec_loop_symm", dim, res, steps, symms, P(ps), P(vs), P(phi), P(vel), P(errs), P(first), ctypes.byref(it))
            key = "loop2005/%d/%d/" % (dim, symms)
            assert it.value > 3 and np.isfinite(phi).all() and np.isfinite(vel).all() and np.abs(vel).max() > 0.5, (key, it.value)
            assert errs.max() < 1e-5, (key, errs.max())               # the script's own threshold, met by the reference
            out[key + "iterations"] = np.array([it.value], np.int64)
            out[key + "first"] = first
            out[key + "err"] = errs
            out[key + "phi"] = phi
            for name, a in (("pressureSym", ps), ("velSym", vs), ("vel", vel)):
                if dim == 2:
                    out[key + name] = a
                out[key + name + "/norms"] = np.array([np.abs(a).max(), np.abs(a.astype(np.float64)).sum()], np.float64)
            print(key, "iterations", it.value, "first errors", first, "final error maxima", errs.reshape(4, -1).max(axis=1))
    res, cap = M.LOOP2065["res"], 60000
    cnt, it = ctypes.c_int(0), ctypes.c_int(0)
    pos0, pd, pos1 = np.zeros((cap, 3), f32), np.zeros(cap, f32), np.zeros((cap, 3), f32)
    dens, vm = np.zeros((res, res, res), f32), ctypes.c_float(0)
    call("rec_loop_partio", res, M.LOOP2065["fixedSeed"], cap, ctypes.byref(cnt), P(pos0), P(pd), P(pos1), P(dens), ctypes.byref(vm), ctypes.byref(it))
    n = cnt.value
    pos0, pd, pos1 = pos0[:n], pd[:n], pos1[:n]
    print("loop2065: particles", n, "iterations", it.value, "vel max", vm.value, "moved by at most", np.abs(pos1 - pos0).max(),
          "channel range", pd.min(), pd.max(), "density range", dens.min(), dens.max())
    assert n > 1000 and it.value > 0 and len(np.unique(pd)) > 100 and pd.min() >= 0 and pd.max() <= f32(1.2) and np.abs(pos1 - pos0).max() > 0
    out["loop2065/count"] = np.array([n, it.value], np.int64)
    out["loop2065/velMax"] = np.array([vm.value], f32)
    out["loop2065/pos0#sha"], out["loop2065/pDens#sha"], out["loop2065/pos1#sha"] = (np.array(M.sha(a)) for a in (pos0, pd, pos1))
    out["loop2065/pos1/sample"] = pos1[::M.LOOP2065["every"]].copy()
    out["loop2065/pDens/sample"] = pd[::M.LOOP2065["every"]].copy()
    out["loop2065/density"] = dens


FILE_DIMS = (4, 3, 2, 3)


def record_files(call, out):
    """the reference's files: header fields and payload of each kind, one file kept as a fixture for the reader, and its messages"""
    golden = os.path.join(ROOT, "tests", "golden")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for kind in M.KINDS:
                a = M.rand_grid(FILE_DIMS, kind, "file")
                for ext in ("uni", "raw"):
                    name = "g_%s.%s" % (kind, ext)
                    call("rec_g4_file", KIND[kind], 1, *FILE_DIMS, P(a.copy()), name.encode())
                    raw = gzip.open(name, "rb").read()
                    if ext == "uni":
                        assert raw[:4] == b"M4T3"
                        h = struct.unpack(UNI_HEADER, raw[4:4 + struct.calcsize(UNI_HEADER)])
                        out["file/%s/header" % kind] = np.array(h[:6] + (h[7],), np.int64)      # dims, gridType, elementType, bytes, dimT
                        raw = raw[4 + struct.calcsize(UNI_HEADER):]
                    assert raw == a.tobytes(), (kind, ext)                                     # the payload is the bridge's array
                    back = M.garbage(FILE_DIMS, kind)
                    call("rec_g4_file", KIND[kind], 0, *FILE_DIMS, P(back), name.encode())
                    same("file/%s/%s" % (kind, ext), back, a)
            with open("g_vec4.uni", "rb") as f:
                blob = f.read()
            with open(os.path.join(golden, "grid4d_vec4.uni"), "wb") as f:
                f.write(blob)
            a = M.garbage(FILE_DIMS, "real")
            msg = {}
            msg["save_noext"] = first_line(call, "rec_g4_file", 0, 1, *FILE_DIMS, P(a), b"noext")
            msg["save_unknown"] = first_line(call, "rec_g4_file", 0, 1, *FILE_DIMS, P(a), b"g.foo")
            msg["load_noext"] = first_line(call, "rec_g4_file", 0, 0, *FILE_DIMS, P(a), b"noext")
            msg["load_unknown"] = first_line(call, "rec_g4_file", 0, 0, *FILE_DIMS, P(a), b"g.foo")
            msg["load_dim"] = first_line(call, "rec_g4_file", 0, 0, 5, 3, 2, 3, P(M.garbage((5, 3, 2, 3), "real")), b"g_real.uni")
            msg["load_dim4"] = first_line(call, "rec_g4_file", 0, 0, 4, 3, 2, 4, P(M.garbage((4, 3, 2, 4), "real")), b"g_real.uni")
            msg["load_size"] = first_line(call, "rec_g4_file", 0, 0, *FILE_DIMS, P(a), b"g_vec4.uni")
            msg["load_type"] = first_line(call, "rec_g4_file", 1, 0, *FILE_DIMS, P(M.garbage(FILE_DIMS, "int")), b"g_real.uni")
            msg["load_raw"] = first_line(call, "rec_g4_file", 0, 0, 5, 3, 2, 3, P(M.garbage((5, 3, 2, 3), "real")), b"g_real.raw")
            msg["construct_2d"] = first_line(call, "rec_g4_construct", 8, 8, 1, 2, 4)
            msg["construct_no4"] = first_line(call, "rec_g4_construct", 8, 8, 8, 3, -1)
            msg["construct_zero"] = first_line(call, "rec_g4_construct", 8, 8, 8, 3, 0)
        finally:
            os.chdir(cwd)
    for k, v in msg.items():
        print("message", k, "=", repr(v))
        out["message/" + k] = np.array(v)


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    record_ops(call, out)
    record_small(call, out)
    record_interp(call, out)
    record_scripts(call, out)
    record_files(call, out)
    record_pdata(call, out)
    record_harness(call, out)
    record_loops(call, out)
    path = os.path.join(ROOT, "tests", "golden", "grid4d.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
