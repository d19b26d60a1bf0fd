"""Recorder of tests/golden/multigrid_levels.npz: the reference's GridMg, level by level, on the edge shapes of
tests/mg_cases.py (EDGE_SHAPES x KINDS, inputs regenerated from its seeded generators, never stored).  No test runs this; it
needs the reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a scratch
directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch
directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmg_levels_rec.so tools/mg_levels_record.cpp -Loracle/_ref -lmanta_ref -lz -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_mg_levels.py $B/libmg_levels_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction)

Per edge case <kind>_<size> and stage system <sys> ("lap": MakeLaplaceMatrix of the kind's flags; "coef", for "gf" and for
fractions_18x18x18: the coefficient system solvePressure builds) the file holds, after GridMg::setA and ONE doVCycle (coarsest
accuracy 1e-8) on the seeded rhs of mg_cases.stage_inputs:
    <case>__<sys>__levels, __size<l>     number of levels, per-level sizes
    <case>__<sys>__type<l>               vertex types (bytes)
    <case>__<sys>__A<l>                  the operator (4 planes on level 0, 14 above; rows of inactive vertices zeroed)
    <case>__<sys>__b<l>, __x<l>          b and x of EVERY level after the V-cycle
    <case>__<sys>__A1fix_idx, _val       "coef" only: the recorded level-1 operator, stored as the entries in which it differs from
                                         the generic-order fp32 sums of tests/mg_model.py's operator1() (flat indices into
                                         (14, n1), values) -- these systems have non-integer entries, so the order in which the
                                         reference sums its sorted paths shows and the model cannot own those bits
and per edge case the solve solvePressure(preconditioner=PcMGDynamic, the kind's arguments):
    <case>__iters, __sha_p, __sha_v      CG iterations, SHA-256 of pressure and corrected velocity
An array of more than 4096 elements is stored as <key>__sha, its SHA-256 digest -- only after tests/mg_model.py reproduced the
array bit for bit here.  (The model is asserted against EVERY recorded array, small ones included, while recording.)"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mg_cases  # noqa: E402
import mg_model as M  # noqa: E402
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

    def put(self, key, arr, model):
        """store arr (or its digest) after the model reproduced it"""
        assert same_bits(arr, model), "%s: the model does not reproduce the reference (%d values differ)" % (
            key, (np.asarray(arr).reshape(-1) != np.asarray(model).reshape(-1)).sum())
        if arr.size > DIGEST_ABOVE:
            self.out[key + "__sha"] = sha(arr)
        else:
            self.out[key] = arr

    def stage(self, tag, dims, A, rhs, integer):
        sx, sy, sz = dims
        A = [np.ascontiguousarray(a, np.float32) for a in A]
        keep = [a.copy() for a in A]
        result = np.zeros((sz, sy, sx), np.float32)
        nl = ctypes.c_int(0)
        self.call("rec_mg_open", sx, sy, sz, P(A[0]), P(A[1]), P(A[2]), P(A[3]), P(rhs), ctypes.c_float(1e-8), P(result), ctypes.byref(nl))
        assert all(same_bits(a, k) for a, k in zip(A, keep)), "setA modified the caller's matrix"
        nl = nl.value
        sizes, t, ops, b, x = [], [], [], [], []
        for l in range(nl):
            s3 = (ctypes.c_int * 3)()
            self.call("rec_mg_size", l, s3)
            sizes.append(tuple(s3))
            n = s3[0] * s3[1] * s3[2]
            arrs = [np.zeros(n, np.uint8), np.zeros((4 if l == 0 else 14, n), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)]
            for what, a in enumerate(arrs):
                self.call("rec_mg_read", l, what, P(a))
            arrs[1][:, arrs[0] == 0] = 0
            t.append(arrs[0]); ops.append(arrs[1]); x.append(arrs[2]); b.append(arrs[3])
        self.call("rec_mg_close")
        assert same_bits(result.reshape(-1), x[0])
        # the model; a non-integer system takes the recorded level-1 operator, stored as its differences from the model's sums
        fix = None
        if nl > 1 and not integer:
            op = M.operator1(sizes[0], t[0], M.activate(sizes[0], *A)[1], sizes[1], t[1])[0]
            idx = np.nonzero(op.reshape(-1).view(np.int32) != ops[1].reshape(-1).view(np.int32))[0].astype(np.int32)
            fix = (idx, ops[1].reshape(-1)[idx].copy())
        H = M.setup(dims, A, A1_patch=fix)      # raises on an integer system whose level-1 sums are not exact
        cyc = M.vcycle(H, rhs)
        assert H.sizes == sizes == mg_cases.EDGE_LEVELS.get(tuple(dims), sizes), (tag, H.sizes, sizes)
        self.out[tag + "__levels"] = np.array(nl, np.int32)
        for l in range(nl):
            self.out[tag + "__size%d" % l] = np.array(sizes[l], np.int32)
            self.put(tag + "__type%d" % l, t[l], H.t[l])
            ma = H.A[l].copy()
            ma[:, H.t[l] == 0] = 0
            self.put(tag + "__A%d" % l, ops[l], ma)
            self.put(tag + "__b%d" % l, b[l], cyc["b"][l])
            self.put(tag + "__x%d" % l, x[l], cyc["x"][l])
        if fix is not None:
            self.out[tag + "__A1fix_idx"], self.out[tag + "__A1fix_val"] = fix
        print("%-28s levels %d active %s coarsest CG %d%s" % (tag, nl, H.active, cyc["cg_iters"], "" if fix is None else "  level-1 entries that differ from the model's order: %d" % len(fix[0])))

    def solve(self, kind, dims):
        sx, sy, sz = dims
        name = mg_cases.case_name(kind, dims)
        flags, vel, phi, kw = mg_cases.inputs(kind, dims)
        v = vel.copy()
        p, rhs = np.zeros((sz, sy, sx), np.float32), np.zeros((sz, sy, sx), np.float32)
        A = [np.zeros((sz, sy, sx), np.float32) for _ in range(4)]
        it = ctypes.c_int(-1)
        self.call("rec_solve", sx, sy, sz, P(flags), P(v), P(p), P(rhs), P(phi), None, ctypes.c_float(kw["cgAccuracy"]), int(kw.get("useL2Norm", False)),
                  int(kw.get("zeroPressureFixing", False)), P(A[0]), P(A[1]), P(A[2]), P(A[3]), ctypes.byref(it))
        want = mg_cases.run_ref(dims, flags, vel, phi, **kw)      # the reference's own solvePressure
        assert same_bits(p, want["pressure"]) and same_bits(v, want["vel"]), name + ": the driven solve is not solvePressure"
        assert np.isfinite(p).all() and it.value < 100, (name, it.value)
        self.out[name + "__iters"] = np.array(it.value, np.int32)
        self.out[name + "__sha_p"], self.out[name + "__sha_v"] = sha(p), sha(v)
        print("%-28s solve: %d iterations" % (name, it.value))
        return A


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    assert util.have_ref()
    R = Recorder(libpath)
    for kind, dims in mg_cases.EDGE_CASES:
        name = mg_cases.case_name(kind, dims)
        A_solve = R.solve(kind, dims)
        for sysname, flags, A, rhs in mg_cases.edge_stage_systems(kind, dims):
            if sysname == "coef":
                assert all(same_bits(a, b) for a, b in zip(A, A_solve)), name + ": the checker library's coefficient system is not the reference's"
            else:
                ref_A = [np.zeros_like(A[0]) for _ in range(4)]
                util.refcall("ref_make_laplace_matrix", dims[0], dims[1], dims[2], flags, ref_A[0], ref_A[1], ref_A[2], ref_A[3], None)
                assert all(same_bits(a, b) for a, b in zip(A, ref_A)), name + ": the checker library's Laplace matrix is not the reference's"
            R.stage("%s__%s" % (name, sysname), dims, A, rhs, integer=(sysname == "lap"))
    dims = mg_cases.FRACTIONS_EDGE_DIMS
    flags, fr, A, rhs = mg_cases.fractions_edge_system()
    ref_A = [np.zeros_like(A[0]) for _ in range(4)]
    util.refcall("ref_make_laplace_matrix", dims[0], dims[1], dims[2], flags, ref_A[0], ref_A[1], ref_A[2], ref_A[3], fr)
    assert all(same_bits(a, b) for a, b in zip(A, ref_A)), "fractions: the checker library's matrix is not the reference's"
    R.stage("fractions_%dx%dx%d__coef" % dims, dims, A, rhs, integer=False)
    path = mg_cases.LEVELS_GOLDEN
    np.savez_compressed(path, **R.out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(R.out), os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main(sys.argv[1])
