"""Recorder of tests/golden/mlflip.npz: the reference's outputs for the cases of tests/mlflip_model.py (inputs are regenerated from its
seeded generators, never stored) and for the recorded dam-break loop with the per-frame calls of the MLFLIP data generation.  No test
runs this; it needs the reference checkout and the build of oracle/ref.mk.  Everything derived from the reference's text stays in a
scratch directory outside the tree.  Run on the CPU machine with one OpenMP thread (REF: the reference checkout, B: any scratch
directory):

    make -f oracle/ref.mk                      # oracle/_ref/libmanta_ref.so and the reference's `prep`
    mkdir -p $B/plugin
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/tfplugins.cpp $B/plugin/tfplugins.cpp
    oracle/_ref/build/prep generate 0 OPENMP $REF/source/ plugin/numpyconvert.cpp $B/plugin/numpyconvert.cpp
    PP=oracle/_ref/build/pp/source
    g++ -O3 -DNDEBUG -DNOPYTHON=1 -DMANTA_MT=1 -DOPENMP=1 -fopenmp -fPIC -std=c++14 -w \\
        -I$B -I$PP -I$PP/util -I$PP/fileio -I$REF/source/nopython -I$REF/source/util -I$REF/source/fileio -I$REF/dependencies/cnpy \\
        -shared -o $B/libmlflip_rec.so tools/mlflip_record.cpp -Loracle/_ref -lmanta_ref -Wl,-rpath,$PWD/oracle/_ref
    OMP_NUM_THREADS=1 python tools/record_mlflip.py $B/libmlflip_rec.so

(the compiler flags are those of oracle/ref.mk: -O3, no -march, so no contraction; tools/mlflip_record.cpp declares the array container
the two plugin files take and includes their expanded text from $B)

Before anything is written the recorder asserts that the numpy model reproduces every recorded array bit for bit (the loop excepted: it
goes through the whole FLIP step, which has its own fixtures).  The reference's flood fill recurses once per cell, so every recorded
region stays under 20 000 cells; the recorder runs in a thread with a large stack all the same.

The file holds copy/to_grid/<kind>/<dtype>, copy/to_array/<kind>/<dtype>, copy/pdata_vec3, simple, feat/<case>,
region/<case>/{r, count, rcnt, ext, marked} and loop/{counts, np, fv<step>, fvhead<step>, labels<step>, pvel<step>}; arrays of more than
mlflip_model.FULL_LIMIT elements as the SHA-256 of their bytes under <key>#sha.
"""
import ctypes
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mlflip_model as M  # noqa: E402

f32, f64, i32, i64 = np.float32, np.float64, np.int32, ctypes.c_int64
DTYPES = {"i": (0, i32), "f": (1, f32), "d": (2, f64)}
KINDS = {"real": 0, "flag": 1, "levelset": 2, "vec3": 3, "mac": 4}


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def fc(x):
    return ctypes.c_float(float(x))


def dims_of(a):
    return np.array(a.shape, np.int64)


def same(tag, got, want):
    assert M.same(got, want), "%s: the model differs from the reference" % tag


def record_copies(call, out):
    sx, sy, sz = M.COPY_DIMS
    A = M.copy_inputs()
    for kind, code in KINDS.items():
        vec = code >= 3
        gdt = i32 if kind == "flag" else f32
        for key, (dcode, dt) in DTYPES.items():
            if vec and key == "i":
                a = np.zeros((sz, sy, sx, 3), i32)
                g = np.zeros((sz, sy, sx, 3), f32)
                for fn, args in (("rec_array_to_grid", (P(a), 0, i64(a.size), a.ndim, P(dims_of(a)), P(g))),
                                 ("rec_grid_to_array", (P(g), P(a), 0, i64(a.size), a.ndim, P(dims_of(a))))):
                    try:
                        call(fn, code, sx, sy, sz, *args)
                    except RuntimeError as e:
                        assert "unknown/unsupported type of Vec3 Numpy array" in str(e), e
                    else:
                        raise AssertionError("the reference takes an int32 array for a vector grid")
                continue
            src = A["v" + key] if vec else A[key]
            if not vec and key == "f":
                src = src.reshape(src.shape + (1,))                    # the [z][y][x][1] shape passes as well
            g = np.full((sz, sy, sx, 3) if vec else (sz, sy, sx), 9, gdt)
            call("rec_array_to_grid", code, sx, sy, sz, P(src), dcode, i64(src.size), src.ndim, P(dims_of(src)), P(g))
            same("to_grid/%s/%s" % (kind, key), M.array_to_grid(src, M.COPY_DIMS, "vec" if vec else ("int" if kind == "flag" else "real")), g)
            out["copy/to_grid/%s/%s" % (kind, key)] = g
            # back: the grid that the float32 / int32 array gives, into an array of every type
            grid = M.array_to_grid(A["vf"] if vec else (A["i"] if kind == "flag" else A["f"]), M.COPY_DIMS,
                                   "vec" if vec else ("int" if kind == "flag" else "real"))
            arr = np.full(grid.shape, 9, dt)
            call("rec_grid_to_array", code, sx, sy, sz, P(grid), P(arr), dcode, i64(arr.size), arr.ndim, P(dims_of(arr)))
            same("to_array/%s/%s" % (kind, key), M.grid_to_array(grid, dt), arr)
            out["copy/to_array/%s/%s" % (kind, key)] = arr
    src = np.ascontiguousarray(A["vf"].reshape(-1, 3))
    dst = np.full(src.shape, 9, f32)
    call("rec_pdata_vec3", i64(src.shape[0]), P(src), P(dst))
    same("pdata_vec3", src, dst)
    out["copy/pdata_vec3"] = dst
    grid = A["f"].copy()
    arr = np.ascontiguousarray(A["d"].astype(f32).reshape(-1)[:sx * sy + 5])
    call("rec_simple", sx, sy, sz, P(grid), P(arr), i64(arr.size), fc(0.375))
    same("simple", M.simple_numpy_test(A["f"], arr, 0.375), grid)
    out["simple"] = grid
    print("copies done")


def ref_extract(call):
    def extract(kind, dims, grid, pos, pflag, ptype, exclude, window, scale, fv, N_row, off_begin):
        fv = np.ascontiguousarray(fv, f32).copy()
        g = np.ascontiguousarray(grid)
        call("rec_feature", {"vel": 0, "phi": 1, "geo": 2}[kind], dims[0], dims[1], dims[2], P(g), i64(pos.shape[0]), P(np.ascontiguousarray(pos)),
             P(pflag), P(ptype), int(exclude), int(window), fc(scale), P(fv), i64(fv.size), int(N_row), int(off_begin))
        return fv
    return extract


def record_features(call, out):
    for name in M.FEATURE_CASES:
        I = M.feature_inputs(name)
        fv = M.feature_matrix(I, ref_extract(call))
        same("feat/%s" % name, M.feature_matrix(I), fv)
        assert (fv == M.FILL).any() and (fv != M.FILL).any()
        M.put(out, "feat/%s" % name, fv)
        print("feature case", name, fv.shape)


def record_regions(call, out):
    E, K = M.REGION_EXTEND, M.REGION_MARK
    for name in M.REGION_CASES:
        flags = M.region_flags(name)
        assert M.border_free(flags, M.FLUID)
        sz, sy, sx = flags.shape
        r, rcnt, ext, marked = (np.full(flags.shape, -3, i32) for _ in range(4))
        count = ctypes.c_int32(-1)
        call("rec_regions", sx, sy, sz, P(flags), M.FLUID, P(r), ctypes.byref(count), P(rcnt), E["region"], E["exclude"], E["depth"], P(ext),
             K["mark"], K["exclude"], K["th"], P(marked))
        mr, mc = M.regions(flags, M.FLUID)
        assert mc == count.value, (name, mc, count.value)
        same("region/%s/r" % name, mr, r)
        same("region/%s/rcnt" % name, M.regional_counts(flags, M.FLUID), rcnt)
        same("region/%s/ext" % name, M.extend_region(flags, **E), ext)
        same("region/%s/marked" % name, M.mark_small_regions(flags, rcnt, **K), marked)
        assert rcnt.max() < 20000
        out["region/%s/count" % name] = np.array([count.value], i32)
        for key, a in (("r", r), ("rcnt", rcnt), ("ext", ext), ("marked", marked)):
            out["region/%s/%s" % (name, key)] = a.astype(np.int16) if a.max() < 2 ** 15 and a.min() >= -2 ** 15 else a
        print("region case", name, "regions", count.value, "largest", int(rcnt.max()))


def record_loop(call, out):
    C = M.LOOP
    steps, N_row, cap = C["steps"], M.loop_row_width(), 100000
    counts = np.zeros((steps, 4), np.int64)
    par = np.array([C["th"], C["window"], C["scale_num"]], np.int32)
    snap = np.array(C["snaps"], np.int32)
    fv = [np.full(cap * N_row, M.FILL, f32) for _ in range(2)]
    lab = [np.full(cap, -7, i32) for _ in range(2)]
    pv = [np.full(3 * cap, M.FILL, f32) for _ in range(2)]
    n = [i64(0), i64(0)]
    call("rec_loop", C["res"], steps, fc(C["dt"]), P(par), P(counts), P(snap), i64(cap), N_row, ctypes.byref(n[0]), P(fv[0]), P(lab[0]), P(pv[0]),
         ctypes.byref(n[1]), P(fv[1]), P(lab[1]), P(pv[1]))
    print("loop counts (particles, regions, labelled cells, particles with a label):\n", counts)
    out["loop/counts"] = counts
    out["loop/np"] = np.array([n[0].value, n[1].value], np.int64)
    for q, step in enumerate(C["snaps"]):
        m = n[q].value
        rows = fv[q][:m * N_row].reshape(m, N_row)[::C["every"]]
        assert (rows == M.FILL).any() and (rows != M.FILL).any(), "the loop excludes no particle (or all of them)"
        M.put(out, "loop/fv%d" % step, rows)
        out["loop/fvhead%d" % step] = rows[:C["head"]].copy()
        out["loop/labels%d" % step] = lab[q][:m].astype(np.int8)
        M.put(out, "loop/pvel%d" % step, pv[q][:3 * m].reshape(m, 3)[::C["every"]])
        print("snap", step, "particles", m, "labels", np.bincount(lab[q][:m]))


def main(libpath):
    assert os.environ.get("OMP_NUM_THREADS") == "1", "record with OMP_NUM_THREADS=1"
    L = ctypes.CDLL(libpath)
    L.rec_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        if getattr(L, name)(*args):
            raise RuntimeError(L.rec_last_error().decode())

    out = {}
    record_copies(call, out)
    record_features(call, out)
    record_regions(call, out)
    record_loop(call, out)
    path = os.path.join(ROOT, "tests", "golden", "mlflip.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    done = []
    threading.stack_size(512 * 1024 * 1024)
    t = threading.Thread(target=lambda: (main(sys.argv[1]), done.append(True)))
    t.start()
    t.join()
    sys.exit(0 if done else 1)
