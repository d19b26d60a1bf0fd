"""numpy model of the grid operations of include/open/manta_hip_gridops.h, and the seeded inputs of their tests.

Arrays are the numpy bridge's: [z][y][x] for Real / int grids, [z][y][x][3] for Vec3 / MAC grids, float32 / int32.  Every function
returns new arrays and keeps the reference's fp32 evaluation order; the three fp64 sums (getL1, getL2, getGridAvg) are summed serially
in the reference's loop order (x fastest), which is what the reference does with one thread.  tests/golden/gridops.npz holds the
reference's outputs for CASES below (tools/record_gridops.py); inputs are regenerated from the seeds here and never stored.

The bound of the fp64 sums: summing the same n fp64 terms in another order moves the result by at most
delta = n * 2^-53 * sum|term|.
Rounding to fp32, sqrt and the product with 1 / count are monotone, so a device result r and the serial fp64 value v satisfy
f(v - delta) <= r <= f(v + delta) with f the same monotone chain: `sum_bounds`.  Where no fp32 rounding boundary lies within delta of v
the two ends are one float and the result must be equal."""
import os
import zlib

import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gridops.npz")
FLUID, OBSTACLE, EMPTY, INFLOW, OUTFLOW = 1, 2, 4, 8, 16
PERMUTATIONS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def name_of(dims):
    return "%dx%dx%d" % tuple(dims)


def rng(*tag):
    """a generator seeded by the tag's text: the same on every machine and in every order of use"""
    return np.random.RandomState(zlib.crc32(repr(tag).encode()) & 0x7FFFFFFF)


def shape_of(dims, ncomp=1):
    sx, sy, sz = dims
    return (sz, sy, sx) if ncomp == 1 else (sz, sy, sx, ncomp)


def same(a, b):
    """bit for bit, NaN payloads and signed zeros included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def in_range(dims, bnd):
    """[z][y][x] mask of FOR_IJK_BND / KERNEL(bnd): z is cut on 3-D grids only"""
    sx, sy, sz = dims
    m = np.zeros(shape_of(dims), bool)
    if sx - 2 * bnd <= 0 or sy - 2 * bnd <= 0 or (sz > 1 and sz - 2 * bnd <= 0):
        return m
    zs = slice(bnd, sz - bnd) if sz > 1 else slice(0, 1)
    m[zs, bnd:sy - bnd, bnd:sx - bnd] = True
    return m


def lower(a, axis):
    """the value of the lower neighbour along grid axis 0 (x), 1 (y), 2 (z); wraps at the side, where nobody looks"""
    return np.roll(a, 1, axis=2 - axis)


def upper(a, axis):
    return np.roll(a, -1, axis=2 - axis)


# ---- permutation ---------------------------------------------------------------------------------------------------------------------
def permute(a, ax):
    """target(s[ax0], s[ax1], s[ax2]) = self(s0, s1, s2); grid axis q is numpy axis 2 - q"""
    order = [2 - ax[2], 2 - ax[1], 2 - ax[0]] + ([3] if a.ndim == 4 else [])
    return np.ascontiguousarray(np.transpose(a, order))


def inverse(ax):
    inv = [0, 0, 0]
    for n, q in enumerate(ax):
        inv[q] = n
    return tuple(inv)


def target_dims(dims, ax):
    return (dims[ax[0]], dims[ax[1]], dims[ax[2]])


def permute_refusal(dims, out_dims, ax):
    """None where permuteAxesCopyToGrid runs, "assert" where the reference's own assert stops it, "outside" where the reference would
    write outside `out`"""
    if any(out_dims[ax[q]] != dims[q] for q in range(3)):
        return "assert"
    if (dims[2] == 1 or out_dims[2] == 1) and ax[2] != 2:
        return "outside"
    if any(out_dims[q] != dims[ax[q]] for q in range(3)):
        return "outside"
    return None


def distinct(dims, kind):
    """a grid of distinct integers (exact in fp32), so that a misplaced word shows"""
    n = dims[0] * dims[1] * dims[2]
    if kind == "int":
        return (np.arange(n, dtype=i32) * 3 - 7).reshape(shape_of(dims))
    if kind == "real":
        return (np.arange(n, dtype=f32) + f32(1)).reshape(shape_of(dims))
    return (np.arange(3 * n, dtype=f32) - f32(n)).reshape(shape_of(dims, 3))


PERMUTE_INPLACE = [(33, 33, 33), (5, 5, 5)]
PERMUTE_COPY = [((31, 34, 5), (1, 0, 2)), ((37, 6, 3), (2, 1, 0)), ((9, 4, 35), (0, 2, 1)), ((64, 32, 1), (1, 0, 2)), ((35, 35, 1), (1, 0, 2))]
PERMUTE_RECORDED_INPLACE = [(5, 5, 5)]          # the fixture holds these for every permutation and kind; 33^3 is the model's alone
KINDS = ["real", "int", "vec"]


# ---- norms ---------------------------------------------------------------------------------------------------------------------------
NORM_DIMS = [(33, 7, 5), (12, 9, 1)]
NORM_BNDS = [0, 1, 3]
NORM_FILLS = ["quarters", "random", "zero"]
NORM_BIG = (129, 127, 64)       # 1048512 cells: 512 blocks of the reduction and a ragged last one


def norm_input(dims, kind, fill):
    r = rng("norm", dims, kind, fill)
    shp = shape_of(dims, 3 if kind == "vec" else 1)
    if fill == "zero":
        return np.zeros(shp, i32 if kind == "int" else f32)
    if kind == "int":
        return r.randint(-8, 9, shp).astype(i32) if fill == "quarters" else r.randint(-30000, 30001, shp).astype(i32)
    if fill == "quarters":
        return (r.randint(-32, 33, shp).astype(f32) / f32(4)).astype(f32)       # multiples of 1/4, |x| <= 8
    return ((r.rand(*shp) - 0.5) * 20).astype(f32)


def norm3(v):
    """norm(Vector3D<float>), vectorbase.h:385-389"""
    l = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    eps2 = f32(1e-6) * f32(1e-6)
    out = np.sqrt(l).astype(f32)
    out = np.where(np.abs(l.astype(f64) - 1.) < f64(eps2), f32(1), out)
    return np.where(l <= eps2, f32(0), out).astype(f32)


def norm_terms(a, bnd, l2):
    """the fp32 terms of getL1 / getL2 in the reference's loop order"""
    dims = (a.shape[2], a.shape[1], a.shape[0])
    m = in_range(dims, bnd)
    if a.dtype == i32:
        t = (a * a).astype(f32) if l2 else np.abs(a).astype(f32)
    elif a.ndim == 4:
        t = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]).astype(f32) if l2 else norm3(a)
    else:
        t = (a * a).astype(f32) if l2 else np.abs(a)
    return t[m]


def serial_sum(t):
    """the reference's `double accu; accu += term` loop"""
    return f64(np.cumsum(t.astype(f64))[-1]) if t.size else f64(0)


def norm(a, bnd, l2):
    s = serial_sum(norm_terms(a, bnd, l2))
    return f32(np.sqrt(s)) if l2 else f32(s)


def sum_delta(t):
    return t.size * 2.0 ** -53 * float(np.abs(t.astype(f64)).sum())


def sum_bounds(t, finish):
    """(lo, hi) of a device result whose fp64 sum of the terms t ran in another order; finish: the monotone chain after the sum"""
    s, d = serial_sum(t), sum_delta(t)
    return finish(f64(s - d)), finish(f64(s + d))


def norm_bounds(a, bnd, l2):
    """the terms of a norm are not negative, and neither is any sum of them: the lower end does not pass 0"""
    return sum_bounds(norm_terms(a, bnd, l2), (lambda s: f32(np.sqrt(max(s, 0.)))) if l2 else (lambda s: f32(max(s, 0.))))


def exactly_summable(kind, fill, l2):
    """the terms are multiples of 2^-4 below 2^8 (or zero): every partial sum of fewer than 2^40 of them is exact in fp64"""
    return fill == "zero" or (fill == "quarters" and (l2 or kind != "vec"))


# ---- join ----------------------------------------------------------------------------------------------------------------------------
def join_inputs(dims, kind):
    r = rng("join", dims, kind)
    shp = shape_of(dims, 3 if kind == "vec" else 1)
    if kind == "int":
        return r.randint(-5, 6, shp).astype(i32), r.randint(-5, 6, shp).astype(i32)
    a, b = (r.randint(-6, 7, shp) / 2.0).astype(f32), (r.randint(-6, 7, shp) / 2.0).astype(f32)       # many ties, some -0 / +0 pairs
    a[r.rand(*shp) < 0.05] = f32(-0.0)
    return a, b


def join(a, b, keepMax):
    """std::max(a, b) = (a < b) ? b : a; std::min(a, b) = (b < a) ? b : a"""
    if a.ndim == 4:
        a1 = a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]
        b1 = b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1] + b[..., 2] * b[..., 2]
        v = np.where(a1 < b1, b1, a1) if keepMax else np.where(b1 < a1, b1, a1)
        return np.repeat(v[..., None], 3, axis=3).astype(f32)
    return (np.where(a < b, b, a) if keepMax else np.where(b < a, b, a)).astype(a.dtype)


# ---- force fields --------------------------------------------------------------------------------------------------------------------
FORCE_DIMS = [(9, 8, 7), (33, 5, 4), (12, 9, 1)]


def random_flags(dims, *tag):
    """fluid, empty and obstacle cells with a few inflow / outflow bits"""
    r = rng("flags", dims, tag)
    f = r.choice([FLUID, EMPTY, OBSTACLE, FLUID | INFLOW, EMPTY | OUTFLOW], size=shape_of(dims), p=[0.4, 0.3, 0.2, 0.05, 0.05])
    return f.astype(i32)


def force_inputs(dims):
    r = rng("force", dims)
    vel = ((r.rand(*shape_of(dims, 3)) - 0.5) * 4).astype(f32)
    force = ((r.rand(*shape_of(dims, 3)) - 0.5) * 3).astype(f32)          # both signs: both arms of the clamp
    region = r.choice([-1.0, 0.0, 0.5, 2.0], size=shape_of(dims)).astype(f32)
    return random_flags(dims, "force"), vel, force, region


def _faces(flags, c):
    cur = (flags & FLUID) != 0
    lo = lower(flags, c)
    return ((lo & FLUID) != 0) | (cur & ((lo & EMPTY) != 0))


def force_field(flags, vel, force, region, additive, isMAC):
    dims = (flags.shape[2], flags.shape[1], flags.shape[0])
    cell = in_range(dims, 1) & ((flags & (FLUID | EMPTY)) != 0)
    if region is not None:
        cell &= ~(region > 0)
    out = vel.copy()
    for c in range(3 if dims[2] > 1 else 2):
        fc = force[..., c]
        fv = fc if isMAC else (f32(0.5) * (lower(fc, c) + fc)).astype(f32)
        w = cell & _faces(flags, c)
        out[..., c] = np.where(w, (vel[..., c] + fv) if additive else fv, vel[..., c])
    return out


def add_force_if_lower(flags, vel, force):
    dims = (flags.shape[2], flags.shape[1], flags.shape[0])
    cell = in_range(dims, 1) & ((flags & (FLUID | EMPTY)) != 0)
    out = vel.copy()
    for c in range(3 if dims[2] > 1 else 2):
        fc, v = force[..., c], vel[..., c]
        fv = (f32(0.5) * (lower(fc, c) + fc)).astype(f32)
        lo, hi = np.where(fv < v, fv, v), np.where(v < fv, fv, v)
        s = (v + fv).astype(f32)
        r = np.where(fv > 0, np.where(hi < s, hi, s), np.where(s < lo, lo, s))
        out[..., c] = np.where(cell & _faces(flags, c), r, v)
    return out


# ---- extrapolateVec3Simple -----------------------------------------------------------------------------------------------------------
EXTRAP_DIMS = [(12, 11, 10), (14, 13, 1)]
EXTRAP_DISTANCES = [1, 2, 5]
EXTRAP_PHIS = ["blob", "none", "all"]


def extrap_inputs(dims, which):
    r = rng("extrap", dims)
    vel = ((r.rand(*shape_of(dims, 3)) - 0.5) * 4).astype(f32)
    vel[r.rand(*shape_of(dims, 3)) < 0.1] = f32(-0.0)
    sx, sy, sz = dims
    z, y, x = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    d = np.sqrt((x - 0.45 * sx) ** 2 + (y - 0.5 * sy) ** 2 + ((z - 0.4 * sz) ** 2 if sz > 1 else 0))
    phi = (d - 0.22 * min(sx, sy)).astype(f32)             # negative inside a small ball, positive outside
    if which == "none":                                    # nothing marked whichever way it marches
        phi = np.zeros_like(phi)
    elif which == "all":                                   # everything marked for inside = False ...
        phi = -np.abs(phi) - f32(1)
    return vel, phi


def extrap_phi(dims, which, inside):
    """... and for inside = True the sign that marks is the other one"""
    vel, phi = extrap_inputs(dims, which)
    return vel, (-phi if (which == "all" and inside) else phi)


def extrapolate_vec3_simple(vel, phi, distance, inside):
    dims = (phi.shape[2], phi.shape[1], phi.shape[0])
    interior = in_range(dims, 1)
    axes = 3 if dims[2] > 1 else 2
    nbv = [fn for c in range(axes) for fn in ((lambda a, c=c: upper(a, c)), (lambda a, c=c: lower(a, c)))]     # +x -x +y -y +z -z
    tmp = np.where(interior & ((phi > 0) if inside else (phi < 0)), 1, 0).astype(i32)
    near = np.zeros(tmp.shape, bool)
    for nb in nbv:
        near |= nb(tmp) == 1
    tmp = np.where(interior & (tmp == 0) & near, 2, tmp).astype(i32)
    out = vel.copy()
    for d in range(2, 1 + distance):
        avg, nbs = np.zeros(vel.shape, f32), np.zeros(tmp.shape, i32)
        for nb in nbv:
            m = nb(tmp) == d
            for c in range(3):
                avg[..., c] = np.where(m, avg[..., c] + nb(out[..., c]), avg[..., c])
            nbs += m
        upd = interior & (tmp == 0) & (nbs > 0)
        div = np.where(nbs > 0, nbs, 1).astype(f32)
        for c in range(3):
            out[..., c] = np.where(upd, (avg[..., c] / div).astype(f32) + f32(0), out[..., c])
        tmp = np.where(upd, d + 1, tmp).astype(i32)
    rest = interior & (tmp == 0)
    out[rest] = f32(0)
    return out


# ---- emission, reset, converters -----------------------------------------------------------------------------------------------------
SMALL_DIMS = [(9, 8, 7), (10, 9, 1)]
EMISSION_CASES = [(False, True, 0), (True, True, 0), (True, False, 0), (True, True, INFLOW), (False, True, INFLOW), (True, False, OUTFLOW),
                  (True, True, INFLOW | OUTFLOW), (False, False, OUTFLOW)]          # (texture given, isAbsolute, type)
RESET_CASES = [("density",), ("density", "heat"), ("density", "fuel", "flame"), ("density", "red", "green", "blue"),
               ("density", "heat", "fuel", "flame", "red", "green", "blue"), ()]
RESET_NAMES = ["density", "heat", "fuel", "flame", "red", "green", "blue"]
RESET_VALUE = f32(-1.25)
SWAPS = [(0, 1, 2), (1, 0, 2), (2, 2, 0), (1, 2, 0)]
MAC_BNDS = [0, 2]
MAC_FLAG = FLUID | INFLOW
INT_FACTOR = f32(0.3)


def real(dims, *tag):
    return ((rng("real", dims, tag).rand(*shape_of(dims)) - 0.5) * 6).astype(f32)


def vec(dims, *tag):
    return ((rng("vec", dims, tag).rand(*shape_of(dims, 3)) - 0.5) * 6).astype(f32)


def emission_texture(dims):
    r = rng("tex", dims)
    return r.choice([0.0, 0.0, -0.0, 0.7, -2.0], size=shape_of(dims)).astype(f32)


def apply_emission(flags, target, source, tex, isAbsolute, type_):
    isIn = ((flags & INFLOW) != 0) if (type_ & INFLOW) else np.zeros(flags.shape, bool)
    isOut = ((flags & OUTFLOW) != 0) if (type_ & OUTFLOW) else np.zeros(flags.shape, bool)
    skip = np.zeros(flags.shape, bool)
    if type_ and tex is not None:
        skip = ~isIn & ~isOut & (tex == 0)
    return np.where(skip, target, source if isAbsolute else (target + source)).astype(f32)


def reset_in_obstacle(flags, vel, grids, value):
    """grids: {name: array} of the given ones; returns (vel, {name: array})"""
    obs = (flags & OBSTACLE) != 0
    v = vel.copy()
    v[obs] = value
    out = {}
    for k, g in grids.items():
        write = k in ("density", "heat", "fuel", "red") or (k == "flame" and "fuel" in grids) or (k in ("green", "blue") and "red" in grids)
        out[k] = np.where(obs & write, value, g).astype(f32)
    return v, out


def copy_mac_data(source, target, flags, flag, bnd):
    dims = (flags.shape[2], flags.shape[1], flags.shape[0])
    m = in_range(dims, bnd) & ((flags & flag) != 0)
    out = target.copy()
    out[m] = source[m]
    return out


def resample_mac_to_vec3(source, target):
    dims = (source.shape[2], source.shape[1], source.shape[0])
    m = in_range(dims, 1)
    out = target.copy()
    for c in range(3):
        if c == 2 and dims[2] == 1:
            cen = np.zeros(m.shape, f32)
        else:
            cen = (f32(0.5) * (source[..., c] + upper(source[..., c], c))).astype(f32)
        out[..., c] = np.where(m, cen, target[..., c])
    return out


def swap_components(vel, c1, c2, c3):
    return np.ascontiguousarray(vel[..., [c1, c2, c3]])


def grid_avg_terms(source, flags):
    return source.reshape(-1) if flags is None else source.reshape(-1)[(flags.reshape(-1) & FLUID) != 0]


def _avg_finish(count):
    return lambda s: f32(f64(s) * (1. / f64(count)))


def grid_avg(source, flags):
    t = grid_avg_terms(source, flags)
    return f32(-1) if t.size == 0 else _avg_finish(t.size)(serial_sum(t))


def grid_avg_bounds(source, flags):
    t = grid_avg_terms(source, flags)
    return (f32(-1), f32(-1)) if t.size == 0 else sum_bounds(t, _avg_finish(t.size))


AVG_FLAGS = ["none", "random", "nofluid"]


def avg_flags(dims, which):
    if which == "none":
        return None
    f = random_flags(dims, "avg")
    return f if which == "random" else np.where((f & FLUID) != 0, EMPTY, f).astype(i32)


def int_input(dims):
    return rng("int", dims).randint(-1000, 1001, shape_of(dims)).astype(i32)


def int_to_real(source, factor):
    return (source.astype(f32) * f32(factor)).astype(f32)


# ---- the cases: (key of the fixture, arguments); the recorder, the model test and the GPU test walk the same lists --------------------
def permute_cases():
    """(key, dims, out_dims or None for permuteAxes, ax, kind)"""
    for dims in PERMUTE_RECORDED_INPLACE:
        for ax in PERMUTATIONS:
            for kind in KINDS:
                yield "perm/in/%s/%d%d%d/%s" % ((name_of(dims),) + ax + (kind,)), dims, None, ax, kind
    for dims, ax in PERMUTE_COPY:
        for kind in KINDS:
            yield "perm/copy/%s/%d%d%d/%s" % ((name_of(dims),) + ax + (kind,)), dims, target_dims(dims, ax), ax, kind
    yield "perm/invalid/5x5x5/011/real", (5, 5, 5), None, (0, 1, 1), "real"             # a repeated axis: nothing happens


def permute_model(dims, out_dims, ax, kind):
    a = distinct(dims, kind)
    if sorted(ax) != [0, 1, 2]:
        return a
    return permute(a, ax)


def out_fill(dims, kind):
    """what `out` holds before permuteAxesCopyToGrid: every cell is overwritten"""
    shp = shape_of(dims, 3 if kind == "vec" else 1)
    return np.full(shp, -77, i32) if kind == "int" else np.full(shp, -77.5, f32)


def norm_cases():
    """(key, dims, kind): the fixture's array is [fill][bnd][l2]"""
    for dims in NORM_DIMS:
        for kind in KINDS:
            yield "norm/%s/%s" % (name_of(dims), kind), dims, kind


def norm_table(dims, kind, fn):
    return np.array([[[fn(norm_input(dims, kind, fill), bnd, l2) for l2 in (0, 1)] for bnd in NORM_BNDS] for fill in NORM_FILLS], f32)


def join_cases():
    for dims in SMALL_DIMS:
        for kind in KINDS:
            for keep in (1, 0):
                yield "join/%s/%s/k%d" % (name_of(dims), kind, keep), dims, kind, keep


def force_cases():
    """(key, dims, with region, isMAC, additive)"""
    for dims in FORCE_DIMS:
        for reg in (0, 1):
            for mac in (0, 1):
                for add in (0, 1):
                    yield "force/%s/r%d/m%d/a%d" % (name_of(dims), reg, mac, add), dims, reg, mac, add


def force_model(dims, reg, mac, add):
    flags, vel, force, region = force_inputs(dims)
    return force_field(flags, vel, force, region if reg else None, add, mac)


def extrap_cases():
    for dims in EXTRAP_DIMS:
        for which in EXTRAP_PHIS:
            for dist in EXTRAP_DISTANCES:
                for inside in (0, 1):
                    yield "extrap/%s/%s/d%d/i%d" % (name_of(dims), which, dist, inside), dims, which, dist, inside


def emission_inputs(dims):
    return random_flags(dims, "emission"), real(dims, "target"), real(dims, "source"), emission_texture(dims)


def reset_inputs(dims):
    return random_flags(dims, "reset"), vec(dims, "reset"), {k: real(dims, "reset", k) for k in RESET_NAMES}


# ---- simple noise --------------------------------------------------------------------------------------------------------------------
NOISE_DIMS = [(10, 9, 8), (11, 10, 1)]
NOISE_SCALE = f32(0.7)
NOISE_SETS = [dict(), dict(posScale=(2.5, 1.5, 0.75), valOffset=0.1, clamp=True, clampNeg=-0.2, clampPos=0.3)]


def noise_field(m, s, nset):
    """a NoiseField of solver s with parameter set nset (the recorder sets the same members on the reference's field)"""
    noise = s.create(m.NoiseField)
    for k, v in NOISE_SETS[nset].items():
        setattr(noise, k, m.vec3(*v) if k == "posScale" else v)
    return noise


def noise_tile_and_params(dims, nset):
    """the wavelet tile (3 x 128^3, bit-exact with the reference's) and the parameter block, from the package on the backend in use"""
    import manta as m
    s = m.Solver(name="n", gridSize=m.vec3(*dims), dim=3 if dims[2] > 1 else 2)
    noise = noise_field(m, s, nset)
    return noise._tile.detach().cpu().numpy().copy(), np.array(list(noise._params()), f32)


def noise_inputs(dims, is_vec):
    flags = random_flags(dims, "noise")
    target = vec(dims, "noise") if is_vec else real(dims, "noise")
    weight = rng("noiseweight", dims).choice([0.0, 0.5, 1.0, -1.5, 2.25], size=shape_of(dims)).astype(f32)
    return flags, target, weight


def noise_cases():
    """(key, dims, vec, with weight, parameter set)"""
    for dims in NOISE_DIMS:
        for is_vec in (0, 1):
            for w in (0, 1):
                for nset in (0, 1):
                    yield "noise/%s/%s/w%d/p%d" % (name_of(dims), "vec" if is_vec else "real", w, nset), dims, is_vec, w, nset


def apply_simple_noise(flags, target, tile, params, scale, weight):
    """target += noise(cell centre) * scale * factor on fluid cells, fp32 products left to right"""
    import obstacle_model
    import turbulence_model
    sz, sy, sx = flags.shape
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    m = (flags & FLUID) != 0
    x, y, z = ((a[m].astype(f32) + f32(0.5)).astype(f32) for a in (i, j, k))
    fac = weight[m] if weight is not None else np.ones(x.shape, f32)
    out = target.copy()
    if target.ndim == 3:
        nv = obstacle_model.noise_evaluate(tile, params, x, y, z)
        out[m] = (target[m] + ((nv * f32(scale)).astype(f32) * fac).astype(f32)).astype(f32)
    else:
        cu = turbulence_model.evaluate_curl(tile, params, np.stack([x, y, z], axis=1))
        for c in range(3):
            out[..., c][m] = (target[..., c][m] + ((cu[:, c] * f32(scale)).astype(f32) * fac).astype(f32)).astype(f32)
    return out


# ---- the legacy single-potential whitewater plugins, secondaryparticles.cpp:549-706 --------------------------------------------------
# The reference addresses neighbours linearly (x + sx * y + strideZ * z, strideZ = 0 in 2-D), and so does this model: a neighbour is a
# roll of the flat arrays.  Inside the preconditions (every itype cell `radius` cells from each side, no visited neighbour on the upper
# outermost layer) no roll wraps.  In 2-D the z loop still runs over -radius .. radius: the plane is met again, with another z in xj.
LEGACY_DIMS = [(12, 10, 9), (14, 12, 1)]
LEGACY_RADII = [1, 2]
LEGACY_TYPES = [(FLUID, FLUID), (FLUID | INFLOW, FLUID | EMPTY)]          # (itype, jtype) of trapped air and wave crest
LEGACY_RATIO_TYPES = [(FLUID, OBSTACLE), (FLUID | INFLOW, OBSTACLE | EMPTY)]
LEGACY_SCALE = f32(1.0 / 12.0)
# (tauMin, tauMax) per type set: the sums of the cases lie below, between and above them (test_gridops_model asserts it per name)
LEGACY_TAU = dict(ta=[(f32(0.5), f32(2.0)), (f32(2.0), f32(16.0))], wc=[(f32(1.0), f32(6.0)), (f32(4.0), f32(30.0))],
                  ke=[(f32(0.2), f32(1.2)), (f32(0.2), f32(1.2))])


def legacy_inputs(dims, radius):
    """flags whose fluid / inflow cells keep `radius` + 1 cells from each side (z too in 3-D), walls on the outermost layer, one fluid
    cell walled in by obstacles (no countable neighbour: NaN ratio); a smooth velocity with noise; normals, part of them near v"""
    import secparts_model as S
    sx, sy, sz = dims
    r = rng("legacy", dims, radius)
    f = r.choice([EMPTY, OBSTACLE, EMPTY | OUTFLOW], size=shape_of(dims), p=[0.6, 0.3, 0.1]).astype(i32)
    core = np.zeros(shape_of(dims), bool)
    m = radius + 1
    zs = slice(m, sz - m) if sz > 1 else slice(0, 1)
    core[zs, m:sy - m, m:sx - m] = True
    pick = r.choice([FLUID, FLUID | INFLOW, EMPTY, OBSTACLE], size=shape_of(dims), p=[0.55, 0.1, 0.2, 0.15]).astype(i32)
    f = np.where(core, pick, f).astype(i32)
    edge = ~in_range(dims, 1)
    f[edge] = OBSTACLE
    # the walled-in cell
    ci, cj, ck = sx // 2, sy // 2, (sz // 2 if sz > 1 else 0)
    zb = slice(ck - radius, ck + radius + 1) if sz > 1 else slice(0, 1)
    f[zb, cj - radius:cj + radius + 1, ci - radius:ci + radius + 1] = OBSTACLE
    f[ck, cj, ci] = FLUID
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    vel = np.stack([np.sin(0.7 * i + 0.3 * j), np.cos(0.5 * j + 0.2 * k), np.sin(0.4 * k + 0.6 * i)], axis=3) * 3 + r.rand(*shape_of(dims, 3))
    vel = vel.astype(f32)
    nrm = S.normalized(((r.rand(*shape_of(dims, 3)) - 0.5) * 2).astype(f32))
    near = r.rand(*shape_of(dims)) < 0.5
    cen = np.nan_to_num(S.centered(vel))
    nrm = np.where(near[..., None], S.normalized((cen + 0.3 * (r.rand(*shape_of(dims, 3)) - 0.5)).astype(f32)), nrm).astype(f32)
    phi = (np.sqrt((i - 0.5 * sx) ** 2 + (j - 0.4 * sy) ** 2 + ((k - 0.5 * sz) ** 2 if sz > 1 else 0)) - 0.3 * sx).astype(f32)
    return f, vel, nrm, phi


def legacy_preconditions(flags, radius, itype, jtype, with_centres=True):
    """what the tests assert of their inputs: every itype cell is `radius` cells from each side, and no jtype cell (a neighbour whose
    getCentered is read) lies on the upper outermost layer"""
    sz, sy, sx = flags.shape
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    it = (flags & itype) != 0
    ok = ((i >= radius) & (i < sx - radius) & (j >= radius) & (j < sy - radius))[it].all()
    if sz > 1:
        ok = ok and ((k >= radius) & (k < sz - radius))[it].all()
    if with_centres:
        upper_layer = (i == sx - 1) | (j == sy - 1) | ((k == sz - 1) if sz > 1 else False)
        ok = ok and not (((flags & (jtype | itype)) != 0) & upper_layer).any()
    return bool(ok)


def _legacy_geometry(flags):
    sz, sy, sx = flags.shape
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return (sx, sy, sz), sx, (sx * sy if sz > 1 else 0), np.stack([i, j, k], axis=1 + 2).reshape(-1, 3)


def _scaled_centres(vel, scale):
    """scaleFromManta * v.getCentered(i, j, k), linear addressing"""
    sz, sy, sx = vel.shape[:3]
    v = vel.reshape(-1, 3)
    Z = sx * sy if sz > 1 else 0
    c = np.zeros(v.shape, f32)
    c[:, 0] = f32(0.5) * (v[:, 0] + np.roll(v[:, 0], -1))
    c[:, 1] = f32(0.5) * (v[:, 1] + np.roll(v[:, 1], -sx))
    if sz > 1:
        c[:, 2] = f32(0.5) * (v[:, 2] + np.roll(v[:, 2], -Z))
    return (f32(scale) * c).astype(f32)


def _legacy_offsets(radius):
    r = range(-radius, radius + 1)
    return [(dx, dy, dz) for dx in r for dy in r for dz in r if (dx, dy, dz) != (0, 0, 0)]


def legacy_gather(mode, flags, vel, normal, radius, tauMin, tauMax, scale, itype, jtype):
    """mode 0 flipComputePotentialTrappedAir, mode 1 flipComputePotentialWaveCrest -> pot"""
    import secparts_model as S
    dims, Y, Z, ijk = _legacy_geometry(flags)
    F = flags.reshape(-1)
    one = f32(1)
    h = f32((1.732 if dims[2] > 1 else 1.414) * radius)
    cell = in_range(dims, 1).reshape(-1) & ((F & itype) != 0)
    xi = (f32(scale) * ijk.astype(f32)).astype(f32)
    vi = _scaled_centres(vel, scale)
    ni = normal.reshape(-1, 3) if normal is not None else None
    acc = np.zeros(F.shape, f32)
    with np.errstate(all="ignore"):
        for dx, dy, dz in _legacy_offsets(radius):
            off = dx + Y * dy + Z * dz
            m = cell & ((np.roll(F, -off) & jtype) != 0)
            xj = (f32(scale) * (ijk + np.array([dx, dy, dz])).astype(f32)).astype(f32)
            xij = (xi - xj).astype(f32)
            fall = (one - (S.norm(xij) / h).astype(f32)).astype(f32)
            if mode == 0:
                vij = (vi - np.roll(vi, -off, axis=0)).astype(f32)
                term = ((S.norm(vij) * (one - S.dot(S.normalized(vij), S.normalized(xij))).astype(f32)).astype(f32) * fall).astype(f32)
            else:
                nj = np.roll(ni, -off, axis=0)
                m = m & (S.dot(S.normalized(xij), ni) < 0)
                term = ((one - S.dot(ni, nj)).astype(f32) * fall).astype(f32)
            acc = np.where(m, (acc + term).astype(f32), acc)
        pot = S.clamp_potential(acc, f32(tauMin), f32(tauMax))
        if mode == 1:
            pot = np.where(S.dot(S.normalized(vi), ni).astype(f64) >= 0.6, pot, f32(0))
    return np.where(cell, pot, f32(0)).astype(f32).reshape(flags.shape), acc.reshape(flags.shape)


def legacy_kinetic(flags, vel, tauMin, tauMax, scale, itype):
    import secparts_model as S
    vi = _scaled_centres(vel, scale)
    ek = (f32(62.5) * S._l2(vi)).astype(f32)
    cell = (flags.reshape(-1) & itype) != 0
    return np.where(cell, S.clamp_potential(ek, f32(tauMin), f32(tauMax)), f32(0)).astype(f32).reshape(flags.shape)


def legacy_ratio(flags, radius, itype, jtype):
    dims, Y, Z, _ = _legacy_geometry(flags)
    F = flags.reshape(-1)
    cell = in_range(dims, 1).reshape(-1) & ((F & itype) != 0)
    cf, cm = np.zeros(F.shape, np.int64), np.zeros(F.shape, np.int64)
    for dx, dy, dz in _legacy_offsets(radius):
        Fq = np.roll(F, -(dx + Y * dy + Z * dz))
        ok = (Fq & jtype) == 0
        cm += ok
        cf += ok & ((Fq & itype) != 0)
    with np.errstate(all="ignore"):
        r = cf.astype(f32) / cm.astype(f32)
    return np.where(cell, r, f32(0)).astype(f32).reshape(flags.shape)


def surface_normals(normal, phi):
    import secparts_model as S
    return S.normalized(S.gradient(normal, phi))


def legacy_cases():
    """(key, dims, radius, type set)"""
    for dims in LEGACY_DIMS:
        for radius in LEGACY_RADII:
            for t in (0, 1):
                yield "legacy/%s/r%d/t%d" % (name_of(dims), radius, t), dims, radius, t


# ---- getInterpolated (host-only), util/interpol.h:52-164 -----------------------------------------------------------------------------
INTERP_KINDS = ["real", "vec", "mac"]


def interp_positions(dims):
    """[n][3] float32: random positions inside, outside on every side (the clamps), on cell centres and faces, on the last cell; on a
    2-D grid z stays below 1, where the reference's index stays in the plane"""
    sx, sy, sz = dims
    r = rng("interp", dims)
    size = np.array(dims, f32)
    p = [r.rand(24, 3) * size, r.rand(8, 3) * (size + 4) - 2]
    edge = [(0, 0, 0), (0.5, 0.5, 0.5), (1, 2, 3), (1.5, 2.5, 0.5), (sx - 1, sy - 1, sz - 1), (sx - 0.5, sy - 0.5, sz - 0.5), (sx - 1.5, 1, 1),
            (sx, sy, sz), (-3, 2.25, 1.75), (2.75, -1, 0.25), (3.25, 4.5, -2), (sx - 1.25, sy - 1.75, 0.75), (sx + 5, 3, 1), (2, sy + 5, 1)]
    p = np.concatenate(p + [np.array(edge, f64)]).astype(f32)
    if sz == 1:
        p[:, 2] = (r.rand(len(p)) * 0.999).astype(f32)
        p[::5, 2] = f32(0.5)
    return p


def _interp_axis(p, size, on_index, cut_upper):
    with np.errstate(invalid="ignore"):
        i = np.trunc(p).astype(np.int64)
    w1 = (p - i.astype(f32)).astype(f32)
    w0 = (1. - w1.astype(f64)).astype(f32)
    lo = p < 0
    i, w0, w1 = np.where(lo, 0, i), np.where(lo, f32(1), w0), np.where(lo, f32(0), w1)
    if cut_upper:
        hi = (i >= size - 1) if on_index else (p >= f32(size - 1))
        i, w0, w1 = np.where(hi, size - 2, i), np.where(hi, f32(0), w0), np.where(hi, f32(1), w1)
    return i, w0.astype(f32), w1.astype(f32)


def interpolate(a, pos, mac):
    """getInterpolated of a Real grid ([n]), a Vec3 grid or, with mac, a MAC grid ([n][3]) at pos [n][3]"""
    sz, sy, sx = a.shape[:3]
    dims = (sx, sy, sz)
    Z = sx * sy if sz > 1 else 0
    pos = np.asarray(pos, f32)
    ax = [_interp_axis((pos[:, c] - f32(0.5)).astype(f32), dims[c], False, c < 2 or sz > 1) for c in range(3)]
    sh = [_interp_axis(pos[:, c], dims[c], True, c < 2 or sz > 1) for c in range(3)]
    planes = a.reshape(-1, 1) if a.ndim == 3 else a.reshape(-1, 3)
    out = []
    for c in range(planes.shape[1]):
        (xi, s0, s1), (yi, t0, t1), (zi, f0, f1) = [(sh if (mac and q == c) else ax)[q] for q in range(3)]
        base = (zi * sy + yi) * sx + xi if mac else xi + sx * yi + Z * zi
        assert (base >= 0).all() and (base + 1 + sx + Z < planes.shape[0]).all()
        d = planes[:, c]
        m = lambda x, w: (x * w).astype(f32)
        lower = (m((m(d[base], t0) + m(d[base + sx], t1)).astype(f32), s0) + m((m(d[base + 1], t0) + m(d[base + 1 + sx], t1)).astype(f32), s1)).astype(f32)
        upper_ = (m((m(d[base + Z], t0) + m(d[base + sx + Z], t1)).astype(f32), s0)
                  + m((m(d[base + 1 + Z], t0) + m(d[base + 1 + sx + Z], t1)).astype(f32), s1)).astype(f32)
        out.append((m(lower, f0) + m(upper_, f1)).astype(f32))
    return out[0] if a.ndim == 3 else np.stack(out, axis=1)


def interp_cases():
    """(key, dims, kind)"""
    for dims in SMALL_DIMS:
        for kind in INTERP_KINDS:
            yield "interp/%s/%s" % (name_of(dims), kind), dims, kind


def interp_input(dims, kind):
    return real(dims, "interp") if kind == "real" else vec(dims, "interp", kind)


NPZ_DIMS = (7, 5, 3)          # the grid whose .npz file getNpzFileSize is asked about: arr_0 is [z][y][x]
