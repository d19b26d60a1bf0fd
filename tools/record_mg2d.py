"""Recorder of tests/golden/mg2d.npz: the reference's GridMg in its 2-D mode, level by level, on the shapes of tests/mg2d_cases.py
(SHAPES x KINDS and the fractions case; inputs regenerated from the seeded generators, never stored), whole solves, and three scene
loops.  No test runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's
text stays in a scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout,
B: any scratch directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/fluidguiding.cpp $B/plugin/fluidguiding.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmg2d_rec.so $B/plugin/fluidguiding.cpp tools/mg2d_record.cpp \\
        -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_mg2d.py $B/libmg2d_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Per case <kind>_<size> and stage system <sys> ("lap": MakeLaplaceMatrix of the kind's flags; "coef", for "gf" and for the fractions
case: the coefficient system solvePressure builds) the file holds, after GridMg::setA and ONE doVCycle (coarsest accuracy 1e-8) on
the seeded rhs of mg_cases.stage_inputs:
    <case>__<sys>__levels, __size<l>     number of levels, per-level sizes
    <case>__<sys>__type<l>               vertex types (bytes)
    <case>__<sys>__A<l>                  the operator (3 planes on level 0, 5 above; rows of inactive vertices zeroed)
    <case>__<sys>__b<l>, __x<l>          b and x of EVERY level after the V-cycle
    <case>__<sys>__A1fix_idx, _val       "coef" only: the recorded level-1 operator, stored as the entries in which it differs from
                                         the generic-order fp32 sums of the model (flat indices into (5, n1), values)
per case the solve solvePressure(the kind's arguments) with PcMGDynamic and with PcMGStatic (on a fresh solver the two are the
same solve, which is asserted):
    <case>__iters, __sha_p, __sha_v      CG iterations, SHA-256 of pressure and corrected velocity
two PcMGStatic solves with different flags on one solver (mg2d_cases.static_pair) as static/iters, static/a__sha_p, ...;
the sorted level-1 paths of the reference (12 ints per path, see tools/mg2d_record.cpp) as paths, and the three loops:
    plume/cg, vel, density, pressure; guiding/pd, cg, vel, density, pressure; flip/cg, vel, phi, pressure, flags, pos, pvel
An array of more than 4096 elements is stored as <key>__sha, its SHA-256 digest -- only after tests/mg2d_model.py reproduced the
array bit for bit here (loops: there is no model; their arrays are digests that the recorder took from the reference alone).
The recorder asserts that every case of mg2d_cases.CASES converged in fewer than 100 iterations and that every case of
mg2d_cases.EXCLUDED did not."""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mg2d_cases as C  # noqa: E402
import mg2d_loops  # noqa: E402
import mg2d_model as M  # noqa: E402
import mg_cases  # noqa: E402
import util  # noqa: E402

DIGEST_ABOVE = 4096


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Recorder(object):
    def __init__(self, libpath):
        self.L = ctypes.CDLL(libpath)
        self.L.rec_last_error.restype = ctypes.c_char_p
        self.out = {}

    def call(self, name, *args):
        if getattr(self.L, name)(*args):
            raise RuntimeError(self.L.rec_last_error().decode())

    def keep(self, key, arr):
        if arr.size > DIGEST_ABOVE:
            self.out[key + "__sha"] = sha(arr)
        else:
            self.out[key] = arr

    def put(self, key, arr, model):
        """store arr (or its digest) after the model reproduced it"""
        assert same_bits(arr, model), "%s: the model does not reproduce the reference (%d values differ)" % (
            key, (np.asarray(arr).reshape(-1) != np.asarray(model).reshape(-1)).sum())
        self.keep(key, arr)

    def stage(self, tag, dims, A, rhs, integer, levels):
        sx, sy, _ = dims
        A = [np.ascontiguousarray(a, np.float32) for a in A]
        keep = [a.copy() for a in A]
        result = np.zeros((1, sy, sx), np.float32)
        nl = ctypes.c_int(0)
        self.call("rec2_mg_open", sx, sy, P(A[0]), P(A[1]), P(A[2]), P(rhs), ctypes.c_float(1e-8), P(result), ctypes.byref(nl))
        assert all(same_bits(a, k) for a, k in zip(A, keep)), "setA modified the caller's matrix"
        nl = nl.value
        sizes, t, ops, b, x = [], [], [], [], []
        for l in range(nl):
            s3 = (ctypes.c_int * 3)()
            self.call("rec2_mg_size", l, s3)
            sizes.append(tuple(s3))
            n = s3[0] * s3[1] * s3[2]
            arrs = [np.zeros(n, np.uint8), np.zeros((3 if l == 0 else 5, n), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)]
            for what, a in enumerate(arrs):
                self.call("rec2_mg_read", l, what, P(a))
            arrs[1][:, arrs[0] == 0] = 0
            t.append(arrs[0]); ops.append(arrs[1]); x.append(arrs[2]); b.append(arrs[3])
        if "paths" not in self.out:
            npaths = self.L.rec2_mg_paths(None)
            paths = np.zeros((npaths, 12), np.int32)
            self.L.rec2_mg_paths(P(paths))
            self.out["paths"] = paths
        self.call("rec2_mg_close")
        assert same_bits(result.reshape(-1), x[0])
        # the model; a non-integer system takes the recorded level-1 operator, stored as its differences from the model's sums
        fix = None
        if nl > 1 and not integer:
            import mg_model as M3
            n0 = sizes[0][0] * sizes[0][1]
            a0 = M3.activate(sizes[0], A[0].reshape(n0), A[1].reshape(n0), A[2].reshape(n0), np.zeros(n0, np.float32))[1]
            op = M3.operator1(sizes[0], t[0], a0, sizes[1], t[1])[0][:5]
            idx = np.nonzero(op.reshape(-1).view(np.int32) != ops[1].reshape(-1).view(np.int32))[0].astype(np.int32)
            fix = (idx, ops[1].reshape(-1)[idx].copy())
        H = M.setup(dims, A, A1_patch=fix)      # raises on an integer system whose level-1 sums are not exact
        cyc = M.vcycle(H, rhs)
        assert H.sizes == sizes == levels, (tag, H.sizes, sizes, levels)
        self.out[tag + "__levels"] = np.array(nl, np.int32)
        for l in range(nl):
            self.out[tag + "__size%d" % l] = np.array(sizes[l], np.int32)
            self.put(tag + "__type%d" % l, t[l], H.t[l])
            ma = H.A2[l].copy()
            ma[:, H.t[l] == 0] = 0
            self.put(tag + "__A%d" % l, ops[l], ma)
            self.put(tag + "__b%d" % l, b[l], cyc["b"][l])
            self.put(tag + "__x%d" % l, x[l], cyc["x"][l])
        if fix is not None:
            self.out[tag + "__A1fix_idx"], self.out[tag + "__A1fix_val"] = fix
        print("%-28s levels %d active %s coarsest CG %d%s" % (tag, nl, H.active, cyc["cg_iters"], "" if fix is None else "  level-1 entries that differ from the model's order: %d" % len(fix[0])))

    def solve(self, name, dims, flags, vel, phi, fractions, kw, expect_converged=True):
        """-> the system matrix (three planes), or None when the case is an excluded one (asserted not to converge)"""
        sx, sy, _ = dims
        v = vel.copy()
        p, rhs = np.zeros((1, sy, sx), np.float32), np.zeros((1, sy, sx), np.float32)
        A = [np.zeros((1, sy, sx), np.float32) for _ in range(3)]
        it = ctypes.c_int(-1)
        try:
            self.call("rec2_solve", sx, sy, P(flags), P(v), P(p), P(rhs), P(phi), P(fractions), ctypes.c_float(kw["cgAccuracy"]), int(kw.get("useL2Norm", False)),
                      int(kw.get("zeroPressureFixing", False)), P(A[0]), P(A[1]), P(A[2]), ctypes.byref(it))
        except RuntimeError as e:
            if expect_converged or "The CG solver diverged" not in str(e):
                raise
            it.value = 100
        if not expect_converged:
            assert it.value >= 100, "%s is listed as excluded but the reference converged in %d iterations" % (name, it.value)
            print("%-28s excluded: %d iterations" % (name, it.value))
            return None
        for pc in (C.PcMGDynamic, C.PcMGStatic):
            want = mg_cases.run_ref(dims, flags, vel, phi, preconditioner=pc, fractions=fractions, **kw)      # the reference's own solvePressure
            assert same_bits(p, want["pressure"]) and same_bits(v, want["vel"]), "%s: the driven solve is not solvePressure(preconditioner=%d)" % (name, pc)
        assert np.isfinite(p).all() and it.value < 100, (name, it.value)
        self.out[name + "__iters"] = np.array(it.value, np.int32)
        self.out[name + "__sha_p"], self.out[name + "__sha_v"] = sha(p), sha(v)
        print("%-28s solve: %d iterations" % (name, it.value))
        return A

    def static_pair(self):
        (fa, va), (fb, vb) = C.static_pair()
        sx, sy, _ = C.STATIC_DIMS
        va, vb = va.copy(), vb.copy()
        pa, pb = np.zeros((1, sy, sx), np.float32), np.zeros((1, sy, sx), np.float32)
        iters = np.zeros(2, np.int32)
        self.call("rec2_static_pair", sx, sy, P(fa), P(va), P(fb), P(vb), ctypes.c_float(C.STATIC_KW["cgAccuracy"]), int(C.STATIC_KW["zeroPressureFixing"]),
                  P(iters), P(pa), P(pb))
        assert (iters < 100).all() and (iters > 0).all(), iters
        fresh = mg_cases.run_ref(C.STATIC_DIMS, fb, C.static_pair()[1][1], None, preconditioner=C.PcMGDynamic, **C.STATIC_KW)
        assert not same_bits(fresh["pressure"], pb), "the second Static solve equals a fresh one: the case shows nothing"
        self.out["static/iters"] = iters
        for k, (p, v) in zip("ab", ((pa, va), (pb, vb))):
            self.out["static/%s__sha_p" % k], self.out["static/%s__sha_v" % k] = sha(p), sha(v)
        print("static pair: iterations", iters.tolist())

    def loops(self):
        f32 = np.float32
        res, steps = C.PLUME["res"], C.PLUME["steps"]
        n = res * res
        cg = np.zeros(steps, np.int32)
        vel, dens, pres = np.zeros((3, n), f32), np.zeros(n, f32), np.zeros(n, f32)
        self.call("rec2_plume", res, steps, C.PcMGDynamic, P(cg), P(vel), P(dens), P(pres))
        assert (cg < 100).all() and (cg > 0).all(), cg
        self.out["plume/cg"] = cg
        self.keep("plume/vel", aos(vel, (1, res, res))); self.keep("plume/density", dens.reshape(1, res, res)); self.keep("plume/pressure", pres.reshape(1, res, res))
        print("plume: cg", cg.tolist())

        res, steps = C.GUIDING["res0"] * C.GUIDING["scale"], C.GUIDING["steps"]
        n = res * res
        pd, cg, ncg = np.zeros(steps, np.int32), np.zeros(8192, np.int32), ctypes.c_int32(0)
        vel, dens, pres = np.zeros((3, n), f32), np.zeros(n, f32), np.zeros(n, f32)
        self.call("rec2_guiding", C.GUIDING["res0"], C.GUIDING["scale"], steps, P(pd), P(cg), len(cg), ctypes.byref(ncg), P(vel), P(dens), P(pres))
        cg = cg[:ncg.value].copy()
        assert (pd < 200).all(), ("the reference's guiding loop does not meet its criterion", pd)
        assert (cg < 100).all(), cg
        self.out["guiding/pd"], self.out["guiding/cg"] = pd, cg
        self.keep("guiding/vel", aos(vel, (1, res, res))); self.keep("guiding/density", dens.reshape(1, res, res)); self.keep("guiding/pressure", pres.reshape(1, res, res))
        print("guiding: pd", pd.tolist(), "cg", cg.tolist())

        res, steps = C.FLIP["res"], C.FLIP["steps"]
        n = res * res
        pos = mg2d_loops.flip_particles()
        np_ = pos.shape[1]
        pvel, cg = np.zeros((3, np_), f32), np.zeros(steps, np.int32)
        vel, phi, pres, fl = np.zeros((3, n), f32), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int32)
        self.call("rec2_flip", res, steps, C.FLIP["release_after"], C.PcMGStatic, ctypes.c_int64(np_), P(pos), P(pvel), P(cg), P(vel), P(phi), P(pres), P(fl))
        assert (cg < 100).all() and (cg > 0).all(), cg
        self.out["flip/cg"] = cg
        self.keep("flip/vel", aos(vel, (1, res, res))); self.keep("flip/phi", phi.reshape(1, res, res)); self.keep("flip/pressure", pres.reshape(1, res, res))
        self.keep("flip/flags", fl.reshape(1, res, res))
        self.keep("flip/pos", np.ascontiguousarray(pos[:, ::7])); self.keep("flip/pvel", np.ascontiguousarray(pvel[:, ::7]))
        print("flip: cg", cg.tolist(), "particles", np_)


def aos(a, shape):
    """[3][n] -> [z][y][x][3], what Grid.to_numpy() of a MAC grid gives"""
    return np.ascontiguousarray(a.reshape(3, -1).T.reshape(shape + (3,)))


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    assert util.have_ref()
    R = Recorder(libpath)
    for dims, levels in C.SHAPES:
        assert M.level_sizes(dims) == levels, (dims, M.level_sizes(dims))
        for kind in C.KINDS:
            name = C.case_name(kind, dims)
            flags, vel, phi, kw = C.inputs(kind, dims)
            A_solve = R.solve(name, dims, flags, vel, phi, None, kw, expect_converged=name not in C.EXCLUDED)
            if A_solve is None:
                continue
            for sysname, A, rhs in C.stage_systems(kind, dims):
                if sysname == "coef":
                    assert all(same_bits(a, b) for a, b in zip(A, A_solve)), name + ": the checker library's coefficient system is not the reference's"
                else:
                    ref_A = [np.zeros_like(A[0]) for _ in range(4)]
                    util.refcall("ref_make_laplace_matrix", dims[0], dims[1], 1, flags, ref_A[0], ref_A[1], ref_A[2], ref_A[3], None)
                    assert all(same_bits(a, b) for a, b in zip(A, ref_A[:3])) and not ref_A[3].any(), name + ": the checker library's Laplace matrix is not the reference's"
                R.stage("%s__%s" % (name, sysname), dims, A, rhs, sysname == "lap", levels)
    dims = C.FRACTIONS_DIMS
    flags, vel, fr = C.fractions_inputs()
    A_solve = R.solve(C.FRACTIONS_NAME, dims, flags, vel, None, fr, C.FRACTIONS_KW)
    A, rhs = C.fractions_system()
    assert all(same_bits(a, b) for a, b in zip(A, A_solve)), "fractions: the checker library's matrix is not the reference's"
    R.stage(C.FRACTIONS_NAME + "__coef", dims, A, rhs, False, C.FRACTIONS_LEVELS)
    R.static_pair()
    R.loops()
    np.savez_compressed(C.GOLDEN, **R.out)
    print("wrote %s: %d arrays, %d bytes" % (C.GOLDEN, len(R.out), os.path.getsize(C.GOLDEN)))
    assert os.path.getsize(C.GOLDEN) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
