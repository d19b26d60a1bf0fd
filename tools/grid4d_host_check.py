"""Driver of tools/grid4d_host_check.hip (its header has the build line): every per-cell body of mantaflow_amd/csrc/grid4d_cells.h on
the host, serially, under the host sanitizers, on the inputs of tests/grid4d_model.py; every output must equal the model bit for bit
and the program must end clean.  Usage: python tools/grid4d_host_check.py <program>."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid4d_model as M  # noqa: E402

f32 = np.float32


def soa(a, kind):
    """the bridge's array -> component planes"""
    a = np.ascontiguousarray(a)
    return a if M.NCOMP[kind] == 1 else np.ascontiguousarray(np.moveaxis(a, -1, 0))


def planes(words, shape, ncomp, dtype):
    a = words.view(dtype)
    return a.reshape(shape) if ncomp == 1 else np.ascontiguousarray(np.moveaxis(a.reshape((ncomp,) + shape), 0, -1))


def run(prog, tmp, op, dims, arrays, *numbers):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([prog, op] + [str(v) for v in dims] + [fin, fout] + [repr(float(v)) if isinstance(v, (float, np.floating)) else str(int(v)) for v in numbers],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (op, dims, r.returncode, r.stderr[-2000:])
    return np.fromfile(fout, np.uint32)


def same(tag, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), tag


def words_of(kind, v):
    w = np.zeros(4, np.int32)
    v = np.atleast_1d(np.array(v, np.int32 if kind == "int" else f32))
    w[:v.size] = v.view(np.int32)
    return [int(x) for x in w]


def main(prog):
    n = 0
    with tempfile.TemporaryDirectory() as tmp:
        for key, name, dims, kind, op, arg in M.op_cases():
            a, b = M.rand_grid(dims, kind, "a"), M.rand_grid(dims, kind, "b")
            nc, sh, dt = M.NCOMP[kind], M.shape_of(dims), a.dtype
            model = M.run_op(dims, kind, op, arg)
            if op == "setBound":
                out = run(prog, tmp, "bound", dims, [soa(a, kind)], nc, arg, *words_of(kind, M.CONST[kind]))
                same(key, planes(out, sh, nc, dt), model)
            elif op == "setBoundNeumann":
                out = run(prog, tmp, "neumann", dims, [soa(a, kind)], nc, arg)
                same(key, planes(out, sh, nc, dt), model)
            elif kind == "int" and op in M.ELEMENTWISE and op != "setConst":
                which = {"add": 0, "sub": 1, "mult": 2, "addScaled": 3, "addConst": 4, "multConst": 5, "clamp": 6}[op]
                v = M.FACTOR[kind] if op == "addScaled" else M.CONST[kind]
                out = run(prog, tmp, "int", dims, [a, b], which, v, int(M.c_int(M.CLAMP[kind][0])), int(M.c_int(M.CLAMP[kind][1])))
                same(key, planes(out, sh, 1, dt), model)
            elif kind in ("vec3", "vec4") and op in ("getMin", "getMax", "getMaxAbs"):
                out = run(prog, tmp, "norm", dims, [soa(a, kind)], nc).view(f32)
                same(key, np.sqrt(out[0:1] if op == "getMin" else out[1:2]), model)
            elif op == "maxDiff":
                out = run(prog, tmp, "maxdiff", dims, [soa(a, kind), soa(b, kind)], nc, int(kind == "int")).view(np.float64)
                same(key, out.astype(f32), model)
            else:
                continue                  # the flat float operators are entries of the core header
            n += 1
        dims = M.SHAPES["a"]
        for rname, (start, end) in M.REGIONS.items():
            for kind in ("real", "vec4"):
                a = M.rand_grid(dims, kind, "a")
                v = list(np.atleast_1d(np.array(M.REGION_VALUE[kind], f32))) + [f32(0)] * 3
                out = run(prog, tmp, "region", dims, [soa(a, kind)], M.NCOMP[kind], *[f32(x) for x in start], *[f32(x) for x in end], *v[:4])
                same("region " + rname, planes(out, M.shape_of(dims), M.NCOMP[kind], f32), M.set_region(a, dims, start, end, M.REGION_VALUE[kind]))
                n += 1
        for sname, (shape, srct, dd) in M.SLICES.items():
            sd = M.SHAPES[shape]
            dsh = (dd[2], dd[1], dd[0])
            for kind in ("real", "vec4"):
                src = M.rand_grid(sd, kind, "a")
                r = np.random.default_rng(M._seed("slice", sname, kind))
                dst = r.uniform(-9, 9, dsh + ((3,) if kind == "vec4" else ())).astype(f32)
                dstt = r.uniform(-9, 9, dsh).astype(f32) if kind == "vec4" else None
                for with_t in ((False, True) if kind == "vec4" else (False,)):
                    arrays = [soa(src, kind), np.moveaxis(dst, -1, 0) if kind == "vec4" else dst] + ([dstt] if with_t else [])
                    out = run(prog, tmp, "slice", sd, arrays, M.NCOMP[kind], srct, *dd, int(with_t))
                    md, mt = M.get_slice(src, srct, dst, dstt if with_t else None)
                    nd = dst.size
                    same("slice " + sname, planes(out[:nd], dsh, 3 if kind == "vec4" else 1, f32), md)
                    if with_t:
                        same("slice t " + sname, out[nd:].view(f32).reshape(dsh), mt)
                    n += 1
        for kind in ("real", "vec4"):
            cases = [(nm, sd, td, {}) for nm, sd, td in M.INTERP_CHAIN] + [(nm,) + c for nm, c in M.INTERP_CASES.items()]
            for nm, sd, td, kw in cases:
                src = M.rand_grid(sd, kind, "interp")
                fac, off = M.grid_factor(sd, td, **kw)
                out = run(prog, tmp, "interp", sd, [soa(src, kind)], M.NCOMP[kind], *td, *fac, *off)
                same("interp " + nm, planes(out, M.shape_of(td), M.NCOMP[kind], f32), M.interpolate(src, td, **kw))
                n += 1
        for npart in (1, 65, 5000):             # particle data: channels of capacity npart + 7, garbage past the live range
            stride = npart + 7
            for kind in M.PD_KINDS:
                nc = 3 if kind == "vec3" else 1
                a = M.pd_rand(npart, kind, "a")
                buf = np.full((nc, stride), 77, a.dtype)
                buf[:, :npart] = a.reshape(npart, nc).T
                for side, op in ((0, "clampMin"), (1, "clampMax")):
                    v = M.PD_CLAMP[kind][side]
                    word = int(M.c_int(v)) if kind == "int" else int(np.array([v], f32).view(np.int32)[0])
                    out = run(prog, tmp, "pdside", (npart, 1, 1, 1), [buf], side, int(kind == "int"), nc, stride, word).view(a.dtype).reshape(nc, stride)
                    same("pd " + op, np.ascontiguousarray(out[:, :npart].T).reshape(a.shape), M.pd_array_op(kind, op, a, a))
                    assert (out[:, npart:] == 77).all()
                    n += 1
                for what, op in ((1, "sumSquare"), (2, "sumMagnitude")):
                    out = run(prog, tmp, "pdterms", (npart, 1, 1, 1), [buf], what, int(kind == "int"), nc, stride).view(np.float64)
                    same("pd " + op, out.astype(f32), M.pd_terms(kind, op, a))
                    n += 1
            a, b = M.pd_rand(npart, "int", "a"), M.pd_rand(npart, "int", "b")
            same("pd safeDiv", run(prog, tmp, "safediv", (npart, 1, 1, 1), [a, b]).view(np.int32), M.pd_array_op("int", "safeDiv", a, b))
            n += 1
        for shape, axis, sym, bound in M.SYM_CASES:          # the symmetry sweeps, both passes of each
            dims = M.SYM_SHAPES[shape]
            sh = (dims[2], dims[1], dims[0])
            for vec in (False, True):
                for dis in ((0, 6) if vec else (0,)):
                    a = M.sym_input(shape, vec)
                    err0 = np.full(sh, 7.0 if vec else np.nan, f32)
                    out = run(prog, tmp, "sym", dims + (1,), [np.moveaxis(a, -1, 0) if vec else a, err0], int(vec), 1, int(sym), axis, bound, dis)
                    ma, me = M.check_symmetry(dims, a, True, sym, axis, bound, dis)
                    na = a.size
                    same("sym " + shape, planes(out[:na], sh, 3 if vec else 1, f32), ma)
                    same("sym err " + shape, out[na:].view(f32).reshape(sh), me)
                    n += 1
    print("grid4d_host_check: %d runs equal the model bit for bit, no sanitizer report" % n)


if __name__ == "__main__":
    main(sys.argv[1])
