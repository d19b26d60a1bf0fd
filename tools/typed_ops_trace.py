"""One short script over the typed containers of mantaflow_amd/core.py, for a kernel trace or an A/B of two versions of the Python layer
on one build of the library: every operator of the four Grid4* classes on a (4, 3, 2, 3) solver (setBoundNeumann is refused there, an
axis being shorter than 3 cells: its message goes into the digest, and the call runs on a (5, 5, 5, 5) solver), the same over the three
Pdata* classes with 5 live particles in channels of capacity 8 and once more in an empty system, and one save / load round trip of a 3-D
grid, a 4-D grid, a particle-data channel and a particle system.  Prints a SHA-256 over every result.
  rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/typed_ops_trace.py"""
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: both then share the HIP runtime that torch loads)
import manta as m  # noqa: E402

DIMS, N, CAP = (4, 3, 2, 3), 5, 8
H = hashlib.sha256()
RNG = np.random.default_rng(2024)


def put(x):
    """a result into the digest: arrays as their bytes, scalars and vectors as float64, messages as text"""
    if isinstance(x, str):
        H.update(x.encode())
    elif isinstance(x, np.ndarray):
        H.update(np.ascontiguousarray(x).tobytes())
    else:
        H.update(np.asarray(list(x) if isinstance(x, (m.vec3, m.vec4)) else x, np.float64).tobytes())


def rand(shape, is_int):
    return RNG.integers(-50, 50, shape).astype(np.int32) if is_int else RNG.uniform(-2, 2, shape).astype(np.float32)


def value(T, which):
    v = {"a": (0.3, -1.7, 2.1, 0.6), "b": (1.3, -0.7, 0.9, -2.2)}[which]
    return {"Real": v[0], "int": 3 if which == "a" else -2, "Vec3": m.vec3(*v[:3]), "Vec4": m.vec4(*v)}[T]


def grids(solver, dims, neumann):
    sx, sy, sz, st = dims
    for cls in (m.Grid4Real, m.Grid4Int, m.Grid4Vec3, m.Grid4Vec4):
        a, b, c = (solver.create(cls) for _ in range(3))
        shape = (st, sz, sy, sx) + ((a._ncomp,) if a._ncomp > 1 else ())
        A, B = rand(shape, a._T == "int"), rand(shape, a._T == "int")

        def fresh():
            a.from_numpy(A)
            b.from_numpy(B)
        ops = (lambda: a.add(b), lambda: a.sub(b), lambda: a.mult(b), lambda: a.addScaled(b, value(a._T, "b")), lambda: a.setConst(value(a._T, "a")),
               lambda: a.addConst(value(a._T, "a")), lambda: a.multConst(value(a._T, "a")), lambda: a.clamp(-0.6, 0.9), lambda: a.clear(),
               lambda: a.copyFrom(b), lambda: a.swap(b), lambda: a.setBound(value(a._T, "a"), 1), lambda: a.setBound(value(a._T, "b"), 0))
        for op in ops:
            fresh()
            op()
            put(a.to_numpy())
            put(b.to_numpy())
        fresh()
        for r in (a.getMin(), a.getMax(), a.getMaxAbs()):
            put(r)
        try:
            a.setBoundNeumann(neumann)
            put(a.to_numpy())
        except RuntimeError as e:
            put(str(e))
        c.from_numpy(A)
        yield c


def channels(solver, n, cap):
    parts = solver.create(m.BasicParticleSystem)
    for cls in (m.PdataReal, m.PdataInt, m.PdataVec3):
        a, b, flag = parts.create(cls), parts.create(cls), parts.create(m.PdataInt)
        if n:
            parts.resizeAll(n, cap)
        shape = (n, 3) if a._ncomp == 3 else (n,)
        A, B, F = rand(shape, a._T == "int"), rand(shape, a._T == "int"), (np.arange(n, dtype=np.int32) % 3) * 2
        B.reshape(-1)[::4] = 0
        flag.from_numpy(F)

        def fresh():
            a.data.fill_(77)
            a.from_numpy(A)
            b.from_numpy(B)
        ops = (lambda: a.add(b), lambda: a.sub(b), lambda: a.mult(b), lambda: a.safeDiv(b), lambda: a.addScaled(b, value(a._T, "b")),
               lambda: a.setConst(value(a._T, "a")), lambda: a.addConst(value(a._T, "a")), lambda: a.multConst(value(a._T, "a")),
               lambda: a.clamp(-0.6, 0.9), lambda: a.clampMin(-0.5), lambda: a.clampMax(0.5), lambda: a.setConstRange(value(a._T, "b"), 1, 4),
               lambda: a.setConstIntFlag(value(a._T, "b"), flag, 4), lambda: a.copyFrom(b), lambda: a.clear())
        for op in ops:
            fresh()
            op()
            put(a.data.cpu().numpy())
            put(b.to_numpy())
        fresh()
        for r in (a.getMin(), a.getMax(), a.getMaxAbs(), a.sum(), a.sum(flag, 4), a.sumSquare(), a.sumMagnitude()):
            put(r)
        yield parts, a


def main():
    s = m.Solver(name="typed", gridSize=m.vec3(*DIMS[:3]), dim=3, fourthDim=DIMS[3])
    big = m.Solver(name="neumann", gridSize=m.vec3(5, 5, 5), dim=3, fourthDim=5)
    p = m.Solver(name="parts", gridSize=m.vec3(8, 7, 6), dim=3)
    kept = list(grids(s, DIMS, 0))
    for _ in grids(big, (5, 5, 5, 5), 1):
        pass
    live = list(channels(p, N, CAP))
    for _ in channels(p, 0, 0):
        pass
    with tempfile.TemporaryDirectory() as tmp:
        g3 = s.create(m.VecGrid).from_numpy(rand((DIMS[2], DIMS[1], DIMS[0], 3), False))
        parts, vec = live[2]
        parts.set_positions(RNG.uniform(0, 6, (N, 3)).astype(np.float32), np.arange(N, dtype=np.int32))
        for obj, ext in ((g3, "uni"), (g3, "raw"), (kept[3], "uni"), (kept[1], "raw"), (vec, "uni"), (live[1][1], "uni"), (parts, "uni")):
            name = os.path.join(tmp, "f." + ext)
            obj.save(name)
            if obj is parts:
                obj.set_positions(np.zeros((1, 3), np.float32))
                obj.load(name)
                put(obj.get_positions())
                put(obj.get_flags())
            else:
                obj.clear()
                obj.load(name)
                put(obj.to_numpy())
    print("sha256 %s" % H.hexdigest())


main()
