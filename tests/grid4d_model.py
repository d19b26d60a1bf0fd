"""numpy statement of the 4-D grids (source/grid4d.{h,cpp}, util/vector4d.h:393-442 of the reference) with branch counters, and the cases
of tests/golden/grid4d.npz.  Arrays are the numpy bridge's: [t][z][y][x] for Real / int, [t][z][y][x][c] for Vec3 / Vec4, float32 or int32;
every float operation below is one numpy float32 operation, i.e. one rounding, in the reference's order.

The fixture is recorded from the compiled reference by tools/record_grid4d.py, which first asserts that this model reproduces every
array bit for bit.  Arrays of more than FULL_LIMIT elements are kept as the SHA-256 of their bytes under <key>#sha (the limit is lower
than the 4096 of the other fixtures: recorded at 4096 this fixture is 973 438 bytes, and it has to stay below 0.5 MB)."""
import hashlib
import zlib

import numpy as np

f32, f64, i32 = np.float32, np.float64, np.int32
FULL_LIMIT = 1024

KINDS = ("real", "int", "vec3", "vec4")
NCOMP = {"real": 1, "int": 1, "vec3": 3, "vec4": 4}
# (sx, sy, sz, st): odd sizes, a cube, a row longer than a wavefront, more than one block with a tail, and 3^4 where every cell is a
# boundary cell of setBound(w = 1)
SHAPES = {"a": (7, 5, 4, 3), "b": (6, 6, 6, 6), "c": (65, 3, 3, 5), "d": (33, 9, 5, 4), "e": (3, 3, 3, 3)}
# setBoundNeumann needs every axis >= 2w + 3
NEUMANN = {"n0": ((5, 5, 5, 5), 0), "n1": ((5, 5, 5, 5), 1), "n2": ((7, 5, 5, 5), 1), "n3": ((9, 7, 7, 7), 2), "n4": ((9, 7, 8, 7), 0)}

CONST = {"real": 0.3, "int": 3, "vec3": (0.3, -1.7, 2.1), "vec4": (0.3, -1.7, 2.1, 0.6)}
FACTOR = {"real": -0.7, "int": -2, "vec3": (1.3, -0.7, 0.9), "vec4": (1.3, -0.7, 0.9, -2.2)}
CLAMP = {"real": (-0.6, 0.9), "int": (-7.9, 12.9), "vec3": (-0.6, 0.9), "vec4": (-0.6, 0.9)}
BOUND_WIDTHS = (0, 1, 2)
ELEMENTWISE = ("add", "sub", "mult", "setConst", "addConst", "addScaled", "multConst", "clamp")
REDUCTIONS = ("getMin", "getMax", "getMaxAbs", "maxDiff")


def shape_of(dims, kind="real"):
    sx, sy, sz, st = dims
    return (st, sz, sy, sx) + ((NCOMP[kind],) if NCOMP[kind] > 1 else ())


def _seed(*tag):
    return zlib.crc32(repr(tag).encode())


def rand_grid(dims, kind, tag):
    """seeded input: floats in (-2, 2), ints in [-50, 50)"""
    r = np.random.default_rng(_seed(dims, kind, tag))
    if kind == "int":
        return r.integers(-50, 50, shape_of(dims, kind)).astype(i32)
    return r.uniform(-2, 2, shape_of(dims, kind)).astype(f32)


def garbage(dims, kind):
    """what outputs are pre-filled with: NaN, or a large int"""
    return np.full(shape_of(dims, kind), 0x7f7f7f7f if kind == "int" else np.nan, i32 if kind == "int" else f32)


def value_of(kind, v):
    """a T as the array it broadcasts from"""
    if kind == "int":
        return i32(v)
    if kind == "real":
        return f32(v)
    return np.array(v, f32)


def c_int(x):
    """int(Real): truncation toward zero"""
    return i32(int(f32(x)))


# ---- element-wise operators, grid4d.cpp:196-226 and grid4d.h:259-268 -------------------------------------------------------------
def elementwise(kind, op, a, b):
    with np.errstate(over="ignore"):
        if op == "add":
            return a + b
        if op == "sub":
            return a - b
        if op == "mult":
            return a * b
        if op == "setConst":
            return np.broadcast_to(value_of(kind, CONST[kind]), a.shape).astype(a.dtype)
        if op == "addConst":
            return a + value_of(kind, CONST[kind])
        if op == "multConst":
            return a * value_of(kind, CONST[kind])
        if op == "addScaled":
            return a + value_of(kind, FACTOR[kind]) * b           # the product is rounded before the sum
        if op == "clamp":
            lo, hi = CLAMP[kind]
            lo, hi = (c_int(lo), c_int(hi)) if kind == "int" else (f32(lo), f32(hi))
            return np.where(a < lo, lo, np.where(a > hi, hi, a)).astype(a.dtype)
    raise KeyError(op)


def norm_square(a):
    s = a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]
    if a.shape[-1] == 4:
        s = s + a[..., 3] * a[..., 3]
    return s


def reduction(kind, op, a, b=None):
    """getMin / getMax / getMaxAbs as Reals (grid4d.cpp:228-267) and grid4dMaxDiff* as the Real the plugin returns (:352-391)"""
    if op == "maxDiff":
        if kind == "real":
            m = f64(np.abs(a - b).max())
        elif kind == "int":
            m = np.abs(a.astype(f64) - b.astype(f64)).max()
        else:
            d = np.abs(a.astype(f64) - b.astype(f64))
            s = d[..., 0]
            for c in range(1, a.shape[-1]):
                s = s + d[..., c]
            m = s.max()
        return f32(max(m, 0.))
    if kind in ("real", "int"):
        lo, hi = f32(a.min()), f32(a.max())
        return {"getMin": lo, "getMax": hi, "getMaxAbs": max(abs(lo), abs(hi))}[op]
    s = norm_square(a)
    return np.sqrt(f32(s.min())) if op == "getMin" else np.sqrt(f32(s.max()))


# ---- boundaries, grid4d.cpp:299-346 ------------------------------------------------------------------------------------------------
def _axes(dims):
    sx, sy, sz, st = dims
    t, k, j, i = np.meshgrid(np.arange(st), np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return i, j, k, t


def bound_mask(dims, w):
    m = np.zeros(shape_of(dims), bool)
    for q, size in zip(_axes(dims), dims):
        m |= (q <= w) | (q >= size - 1 - w)
    return m


def set_bound(kind, a, dims, w, cnt=None):
    m = bound_mask(dims, w)
    if cnt is not None:
        cnt["bound_cells"] = cnt.get("bound_cells", 0) + int(m.sum())
        cnt["inner_cells"] = cnt.get("inner_cells", 0) + int((~m).sum())
    out = a.copy()
    out[m] = value_of(kind, CONST[kind])
    return out


def set_bound_neumann(a, dims, w, cnt=None):
    """every axis >= 2w + 3 (asserted): the source of a boundary cell is an inner cell, so the in-place kernel is a gather"""
    assert w >= 0 and min(dims) >= 2 * w + 3, (dims, w)
    src = []
    for q, size in zip(_axes(dims), dims):
        s = np.where(q <= w, w + 1, q)
        s = np.where(q >= size - 1 - w, size - 1 - w - 1, s)      # tested second: it wins where both hold
        src.append(s)
    m = bound_mask(dims, w)
    assert not m[src[3], src[2], src[1], src[0]].any()
    if cnt is not None:
        nax = sum(((q <= w) | (q >= size - 1 - w)).astype(int) for q, size in zip(_axes(dims), dims))
        for n in range(5):
            cnt["neumann_axes_%d" % n] = cnt.get("neumann_axes_%d" % n, 0) + int((nax == n).sum())
    return a[src[3], src[2], src[1], src[0]].copy()


# ---- region, slices, components, grid4d.cpp:292-296, 394-433 -------------------------------------------------------------------
def set_region(a, dims, start, end, value, cnt=None):
    start, end = np.array(start, f32), np.array(end, f32)
    m = np.ones(shape_of(dims), bool)
    for c, q in enumerate(_axes(dims)):
        p = q.astype(f32)
        m &= ~((p < start[c]) | (p > end[c]))
    if cnt is not None:
        cnt["region_cells"] = cnt.get("region_cells", 0) + int(m.sum())
    out = a.copy()
    out[m] = np.array(value, f32) if a.ndim == 5 else f32(value)
    return out


def get_slice(src, srct, dst, dstt=None, cnt=None):
    """src [t][z][y][x](,[4]) -> dst [z][y][x](,[3]) (and dstt [z][y][x]) on the cells both have; srct outside the grid: nothing"""
    dst = dst.copy()
    dstt = None if dstt is None else dstt.copy()
    if not 0 <= srct < src.shape[0]:
        if cnt is not None:
            cnt["slice_out_of_range"] = cnt.get("slice_out_of_range", 0) + 1
        return dst, dstt
    z, y, x = (min(a, b) for a, b in zip(src.shape[1:4], dst.shape[:3]))
    if cnt is not None and (z, y, x) != src.shape[1:4]:
        cnt["slice_smaller_dst"] = cnt.get("slice_smaller_dst", 0) + 1
    if src.ndim == 4:
        dst[:z, :y, :x] = src[srct, :z, :y, :x]
    else:
        dst[:z, :y, :x, :] = src[srct, :z, :y, :x, :3]
        if dstt is not None:
            dstt[:z, :y, :x] = src[srct, :z, :y, :x, 3]
    return dst, dstt


def get_comp(src4, c):
    return src4[..., c].copy()


def set_comp(src, dst4, c):
    out = dst4.copy()
    out[..., c] = src
    return out


# ---- interpolation, vector4d.h:393-442 and grid4d.cpp:440-467 ------------------------------------------------------------------------
def grid_factor(sdims, tdims, offset=(0, 0, 0, 0), scale=(1, 1, 1, 1), size=(-1, -1, -1, -1)):
    """gridFactor4d: (srcFac, retOff) in fp32"""
    s1, s2 = np.array(sdims, f32), np.array(tdims, f32)
    off, scale, size = np.array(offset, f32), np.array(scale, f32), np.array(size, f32)
    s2 = np.where(size > 0., size, s2)
    fac = (s1 / s2) / scale
    return fac, -off * fac + fac * f32(0.5)


def _axis_index(pos, size, axis, cnt):
    p = pos - f32(0.5)
    xi = np.trunc(p).astype(np.int64)
    w1 = p - xi.astype(f32)
    w0 = (1. - w1.astype(f64)).astype(f32)
    lo = p < 0.
    xi = np.where(lo, 0, xi)
    w0 = np.where(lo, f32(1), w0)
    w1 = np.where(lo, f32(0), w1)
    hi = xi >= size - 1
    xi = np.where(hi, size - 2, xi)
    w0 = np.where(hi, f32(0), w0)
    w1 = np.where(hi, f32(1), w1)
    if cnt is not None:
        for name, m in (("lower", lo), ("upper", hi), ("centre", (~lo) & (~hi) & (w1 == 0))):
            k = "interp_%s_%s" % (name, axis)
            cnt[k] = cnt.get(k, 0) + int(m.sum())
    return xi, w0.astype(f32), w1.astype(f32)


def interpol4d(data, pos, cnt=None):
    """data [t][z][y][x]; pos = (x, y, z, t) arrays of one shape"""
    st, sz, sy, sx = data.shape
    assert min(data.shape) >= 2
    xi, s0, s1 = _axis_index(pos[0], sx, "x", cnt)
    yi, t0, t1 = _axis_index(pos[1], sy, "y", cnt)
    zi, f0, f1 = _axis_index(pos[2], sz, "z", cnt)
    ti, g0, g1 = _axis_index(pos[3], st, "t", cnt)

    def D(dt, dz, dy, dx):
        return data[ti + dt, zi + dz, yi + dy, xi + dx]

    def cube(dt):
        return (((D(dt, 0, 0, 0) * t0 + D(dt, 0, 1, 0) * t1) * s0 + (D(dt, 0, 0, 1) * t0 + D(dt, 0, 1, 1) * t1) * s1) * f0
                + ((D(dt, 1, 0, 0) * t0 + D(dt, 1, 1, 0) * t1) * s0 + (D(dt, 1, 0, 1) * t0 + D(dt, 1, 1, 1) * t1) * s1) * f1)
    return cube(0) * g0 + cube(1) * g1


def interpolate(source, tdims, offset=(0, 0, 0, 0), scale=(1, 1, 1, 1), size=(-1, -1, -1, -1), cnt=None):
    """interpolateGrid4d / interpolateGrid4dVec: the target array"""
    sdims = source.shape[3], source.shape[2], source.shape[1], source.shape[0]
    fac, off = grid_factor(sdims, tdims, offset, scale, size)
    pos = [q.astype(f32) * fac[c] + off[c] for c, q in enumerate(_axes(tdims))]
    if source.ndim == 4:
        return interpol4d(source, pos, cnt)
    return np.stack([interpol4d(np.ascontiguousarray(source[..., c]), pos, cnt if c == 0 else None) for c in range(source.shape[-1])], axis=-1)


# the interpolation cases: name -> (source dims, target dims, keyword arguments).  "up*/down*" are the chain of the reference's
# test_0042_interpol4d.py at res = 8 (each step reads the step before it; "up1" reads the seeded 4^4 grid).
INTERP_CHAIN = (("up1", (4,) * 4, (8,) * 4), ("up2", (8,) * 4, (16,) * 4), ("down1", (16,) * 4, (8,) * 4), ("down2", (8,) * 4, (4,) * 4))
INTERP_CASES = {
    "ratio_up": ((7, 5, 4, 3), (9, 11, 5, 7), {}),
    "ratio_down": ((9, 11, 5, 7), (7, 5, 4, 3), {}),
    "two_cells": ((2, 5, 2, 3), (5, 4, 6, 5), {}),
    "centre": ((6, 6, 6, 6), (6, 6, 6, 6), {}),                                   # factor 1: every position is a cell centre
    "offset": ((7, 5, 4, 3), (9, 11, 5, 7), {"offset": (0.75, -1.5, 0.25, 1.0)}),
    "scale": ((7, 5, 4, 3), (9, 11, 5, 7), {"scale": (1.5, 0.75, 2.0, 0.5)}),
    "size": ((7, 5, 4, 3), (9, 11, 5, 7), {"size": (12.0, -1.0, 4.0, 7.5)}),
    "all": ((7, 5, 4, 3), (6, 7, 8, 5), {"offset": (-0.5, 0.3, 1.25, -0.7), "scale": (0.8, 1.1, 1.0, 1.3), "size": (7.0, 6.5, -1.0, 4.0)}),
}
REGIONS = {"frac": ((1.5, 0.0, 0.5, 1.0), (4.25, 3.0, 2.5, 1.0)), "all": ((-1, -1, -1, -1), (99, 99, 99, 99)), "none": ((3, 3, 3, 3), (2, 9, 9, 9))}
REGION_VALUE = {"real": 1.75, "vec4": (1.75, -0.3, 0.6, 2.5)}
# (source shape, srct, dst dims): a valid slice, the last one, out of range on both sides, a smaller and a larger dst
SLICES = {"mid": ("a", 1, (7, 5, 4)), "last": ("a", 2, (7, 5, 4)), "below": ("a", -1, (7, 5, 4)), "above": ("a", 3, (7, 5, 4)),
          "smaller": ("a", 0, (5, 5, 3)), "larger": ("a", 1, (9, 6, 5)), "row": ("c", 4, (65, 3, 3))}


# ---- fixture helpers ------------------------------------------------------------------------------------------------------------------
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def put(out, key, a):
    a = np.ascontiguousarray(a)
    if a.size > FULL_LIMIT:
        out[key + "#sha"] = np.array(sha(a))
    else:
        out[key] = a


def same_as_fixture(golden, key, got):
    """None where `got` is the recorded array bit for bit, else a message"""
    got = np.ascontiguousarray(got)
    if key + "#sha" in golden.files:
        return None if sha(got) == str(golden[key + "#sha"]) else "%s: digest differs" % key
    want = golden[key]
    if want.shape != got.shape or want.dtype != got.dtype:
        return "%s: %s %s vs recorded %s %s" % (key, got.shape, got.dtype, want.shape, want.dtype)
    u = "u%d" % got.dtype.itemsize
    d = got.view(u) != want.view(u)
    if d.any():
        at = tuple(np.argwhere(d)[0])
        return "%s: %d of %d words differ, first at %s: %r vs recorded %r" % (key, int(d.sum()), d.size, at, got[at], want[at])
    return None


def op_cases():
    """every (key, shape name, dims, kind, op, argument) of the element-wise, reduction and boundary part of the fixture"""
    for name, dims in SHAPES.items():
        for kind in KINDS:
            for op in ELEMENTWISE + REDUCTIONS:
                yield "op/%s/%s/%s" % (name, kind, op), name, dims, kind, op, None
            for w in BOUND_WIDTHS:
                yield "op/%s/%s/setBound%d" % (name, kind, w), name, dims, kind, "setBound", w
    for name, (dims, w) in NEUMANN.items():
        for kind in KINDS:
            yield "op/%s/%s/setBoundNeumann" % (name, kind), name, dims, kind, "setBoundNeumann", w


def run_op(dims, kind, op, arg, cnt=None):
    """the model's answer for one case of op_cases(): an array, or a float32 scalar"""
    a, b = rand_grid(dims, kind, "a"), rand_grid(dims, kind, "b")
    if op in ELEMENTWISE:
        return elementwise(kind, op, a, b)
    if op in REDUCTIONS:
        return np.array([reduction(kind, op, a, b)], f32)
    if op == "setBound":
        return set_bound(kind, a, dims, arg, cnt)
    if op == "setBoundNeumann":
        return set_bound_neumann(a, dims, arg, cnt)
    raise KeyError(op)


# ---- the sequences of the reference's harness scripts, restated (the scripts themselves are not copied) ------------------------------
# test_0032_grid4dop.py: three grids per element type; g1 = c1 + add, g2 = c2 * mul, g3 = g1 + g2 + half * g2.  Python floats reach
# the reference as Reals.
SCRIPT32_DIMS = (10, 20, 30, 12)
SCRIPT32 = {"real": (1.0, 2.4, 0.1, 0.5, 0.5), "vec3": (1.0, 1.0, 0.2, 0.5, 0.5), "int": (123, 2, 2, 3, 2), "vec4": (1.0, 1.0, 0.2, 0.5, 0.5)}


def script32_model():
    """kind -> the constant value of (g1, g2, g3) at the end of the script's computed branch"""
    out = {}
    for kind, (c1, c2, add, mul, half) in SCRIPT32.items():
        T = i32 if kind == "int" else f32
        g1 = T(c1) + T(add)
        g2 = T(c2) * T(mul)
        g3 = g1 + g2
        g3 = g3 + T(half) * g2
        out[kind] = np.array([g1, g2, g3], T)
    return out


# test_0042_interpol4d.py at res = 8: a block set in the 4^4 grid, interpolated 4 -> 8 -> 16 -> 8 -> 4, scalar and Vec4, and the slices
# at t = 0.5 the script takes for display
SCRIPT42_RES = 8


def script42_model():
    sm, nm, xl = (SCRIPT42_RES // 2,) * 4, (SCRIPT42_RES,) * 4, (SCRIPT42_RES * 2,) * 4
    rs, re = f32(sm[0] * 0.3), f32(sm[0] * 0.7)
    out = {}
    for kind, value, tag in (("real", 1.0, "density"), ("vec4", (1.0, 1.0, 1.0, 1.0), "v3")):
        zero = np.zeros(shape_of(sm, kind), f32)
        out["sm_" + tag] = set_region(zero, sm, (rs,) * 4, (re,) * 4, value)
        out[tag] = interpolate(out["sm_" + tag], nm)
        out["xl_" + tag] = interpolate(out[tag], xl)
        out[tag + "2"] = interpolate(out["xl_" + tag], nm)
        out["sm_" + tag + "2"] = interpolate(out[tag + "2"], sm)
        for name, dims in ((tag, nm), (tag + "2", nm), ("sm_" + tag, sm), ("sm_" + tag + "2", sm), ("xl_" + tag, xl)):
            dsh = (dims[2], dims[1], dims[0])
            dst = np.zeros(dsh + ((3,) if kind == "vec4" else ()), f32)
            out["slice_" + name] = get_slice(out[name], int(dims[0] * 0.5), dst)[0]
    return out


# ---- particle data, particle.cpp:434-673: arrays [n] (Real, int) or [n][3] (Vec3) over the live slots ---------------------------------
PD_KINDS = ("real", "int", "vec3")
PD_SIZES = (0, 1, 63, 64, 65, 5000)
PD_CONST = {"real": 0.3, "int": 3, "vec3": (0.3, -1.7, 2.1)}
PD_FACTOR = {"real": -0.7, "int": -2, "vec3": (1.3, -0.7, 0.9)}
PD_CLAMP = {"real": (-0.6, 0.9), "int": (-7.9, 12.9), "vec3": (-0.6, 0.9)}
PD_FLAG = 4
PD_ARRAY_OPS = ("add", "sub", "mult", "safeDiv", "addConst", "addScaled", "multConst", "clamp", "clampMin", "clampMax", "setConstRange",
                "setConstIntFlag/all", "setConstIntFlag/none", "setConstIntFlag/alternating")
PD_MINMAX = ("getMin", "getMax", "getMaxAbs")
PD_SUMS = ("sum", "sum/all", "sum/none", "sum/alternating", "sumSquare", "sumMagnitude")


def pd_rand(n, kind, tag):
    """seeded channel; `b` channels carry zeros for safeDiv"""
    r = np.random.default_rng(_seed("pd", n, kind, tag))
    shape = (n, 3) if kind == "vec3" else (n,)
    a = r.integers(-50, 50, shape).astype(i32) if kind == "int" else r.uniform(-2, 2, shape).astype(f32)
    if tag == "b" and n:
        a.reshape(-1)[::7] = 0
    return a


def pd_exact(n, kind, tag):
    """exactly summable: multiples of 2^-3 small enough that every partial sum of the values, of their squares (multiples of 2^-6 below
    2^24 * 2^-6 in total) and of their lengths is exact in fp32, in any order.  Vec3 slots are integer vectors of integer length
    (permuted, signed, scaled by 1..3), so that norm() is exact as well"""
    r = np.random.default_rng(_seed("pdx", n, kind, tag))
    if kind != "vec3":
        a = r.integers(-32, 32, n)
        return a.astype(i32) if kind == "int" else (a.astype(f32) * f32(0.125))
    base = np.array([(3, 4, 0), (0, 0, 1), (2, 3, 6), (1, 4, 8), (4, 4, 7), (0, 0, 0), (8, 0, 0)], np.int64)      # lengths 5, 1, 7, 9, 9, 0, 8
    a = base[r.integers(0, len(base), n)] * r.integers(1, 4, (n, 1)) * r.choice((-1, 1), (n, 3))
    a = np.take_along_axis(a, np.argsort(r.random((n, 3)), axis=1), axis=1)
    return a.astype(f32) * f32(0.125)


def pd_flags(n, pattern):
    """an int channel whose `PD_FLAG` bit is set in all, none or every other slot (other bits are noise)"""
    r = np.random.default_rng(_seed("pdt", n, pattern))
    t = (r.integers(0, 4, n) | 8 * r.integers(0, 2, n)).astype(i32)
    if pattern == "all":
        t |= PD_FLAG
    elif pattern == "alternating":
        t[::2] |= PD_FLAG
    return t


def pd_range(n):
    return n // 4, n - n // 3


def pd_array_op(kind, op, a, b, t=None):
    v, f = value_of(kind, PD_CONST[kind]), value_of(kind, PD_FACTOR[kind])
    lo, hi = PD_CLAMP[kind]
    lo, hi = (c_int(lo), c_int(hi)) if kind == "int" else (f32(lo), f32(hi))
    with np.errstate(all="ignore"):
        if op == "add":
            return a + b
        if op == "sub":
            return a - b
        if op == "mult":
            return a * b
        if op == "safeDiv":
            if kind == "int":
                q = np.trunc(a.astype(f64) / np.where(b == 0, 1, b)).astype(i32)      # C division truncates
                return np.where(b != 0, q, a).astype(i32)
            return np.where(b != 0, a / np.where(b != 0, b, f32(1)), a).astype(f32)
        if op == "addConst":
            return a + v
        if op == "multConst":
            return a * v
        if op == "addScaled":
            return a + f * b
        if op == "clamp":
            return np.where(a < lo, lo, np.where(a > hi, hi, a)).astype(a.dtype)
        if op == "clampMin":           # std::max(vmin, x)
            return np.where(lo < a, a, lo).astype(a.dtype)
        if op == "clampMax":           # std::min(vmax, x)
            return np.where(a < hi, a, hi).astype(a.dtype)
        if op == "setConstRange":
            out = a.copy()
            s, e = pd_range(len(a))
            out[s:e] = v
            return out
        if op.startswith("setConstIntFlag"):
            out = a.copy()
            out[(t & PD_FLAG) != 0] = v
            return out
    raise KeyError(op)


def pd_min_max(kind, op, a):
    big = np.finfo(f32).max
    if kind == "vec3":
        s = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
        with np.errstate(invalid="ignore"):
            lo, hi = np.sqrt(f32(s.min()) if len(a) else big), np.sqrt(f32(s.max()) if len(a) else -big)
        return lo if op == "getMin" else hi
    lo, hi = (f32(a.min()), f32(a.max())) if len(a) else (big, -big)
    return {"getMin": lo, "getMax": hi, "getMaxAbs": max(abs(lo), abs(hi))}[op]


def pd_norm3(a):
    """norm(Vec3), vectorbase.h:385-389"""
    l = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
    eps2 = f32(1e-6) * f32(1e-6)
    out = np.sqrt(l)
    out = np.where(np.abs(l.astype(f64) - 1.) < f64(eps2), f32(1), out)
    return np.where(l <= eps2, f32(0), out).astype(f32)


def pd_terms(kind, op, a, t=None):
    """the fp32 (or int) terms a sum adds, slot by slot; [n] or, for the Vec3 sum, [n][3]"""
    what = op.split("/")[0]
    if what == "sum":
        terms = a
        if t is not None:
            terms = a[(t & PD_FLAG) != 0]
        return terms
    with np.errstate(over="ignore"):
        if kind == "vec3":
            return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]) if what == "sumSquare" else pd_norm3(a)
        if kind == "int":
            return (a * a).astype(f32) if what == "sumSquare" else np.abs(a).astype(f32)
        return a * a if what == "sumSquare" else np.abs(a)


def pd_sum_reference(terms):
    """what the reference computes: one thread adding Reals (or ints) in slot order"""
    if terms.dtype == i32:
        with np.errstate(over="ignore"):
            return np.add.accumulate(terms, dtype=i32)[-1:].copy() if len(terms) else np.zeros(1, i32)
    if not len(terms):
        return np.zeros(terms.shape[1:] or (1,), f32)
    return np.atleast_1d(np.add.accumulate(terms, axis=0, dtype=f32)[-1]).astype(f32)


def pd_sum_bound(terms):
    """|any order of fp32 additions - exact| <= gamma(n-1) * sum|term|, plus 2^-24 |S| for the contract's one rounding; per component"""
    import math
    n = len(terms)
    cols = terms.reshape(n, int(np.prod(terms.shape[1:]))).astype(f64)
    u = 2.0 ** -24
    k = max(n - 1, 0)
    gamma = k * u / (1 - k * u)
    exact = np.array([math.fsum(cols[:, c]) for c in range(cols.shape[1])])
    bound = np.array([gamma * math.fsum(np.abs(cols[:, c])) for c in range(cols.shape[1])]) + u * np.abs(exact)
    return exact, bound


def pd_cases():
    """every (key, n, kind, op) of the particle-data part of the fixture"""
    for n in PD_SIZES:
        for kind in PD_KINDS:
            for op in PD_ARRAY_OPS + PD_MINMAX + PD_SUMS:
                yield "pd/%d/%s/%s" % (n, kind, op), n, kind, op
            for op in PD_SUMS:
                yield "pdx/%d/%s/%s" % (n, kind, op), n, kind, op


def pd_inputs(key, n, kind, op):
    exact = key.startswith("pdx/")
    a = pd_exact(n, kind, "a") if exact else pd_rand(n, kind, "a")
    b = pd_rand(n, kind, "b")
    t = pd_flags(n, op.split("/")[1]) if "/" in op else None
    return a, b, t


# ---- checkSymmetry / checkSymmetryVec3 (plugin/initplugins.cpp:189-269) and testInitGridWithPos (plugin/flip.cpp:191-193) -----------
# 3-D arrays are [z][y][x](,[3]); a 2-D grid has one plane
SYM_SHAPES = {"e3": (6, 4, 4), "o3": (7, 5, 3), "e2": (8, 6, 1), "o2": (5, 7, 1), "w": (65, 3, 4)}
SYM_CASES = [(shape, axis, sym, bound) for shape in SYM_SHAPES for axis in (0, 1, 2) for sym in (False, True) for bound in (0, 1)
             if not (SYM_SHAPES[shape][2] == 1 and axis == 2) and not (shape == "w" and axis)]
SYM_DISABLE = (0, 1, 2, 4, 6)


def _in_bounds(dims, p, b):
    sx, sy, sz = dims
    ok = p[0] >= b and p[1] >= b and p[0] < sx - b and p[1] < sy - b
    return ok and ((p[2] >= b and p[2] < sz - b) if sz > 1 else p[2] == 0)


def _sym_sweep_literal(dims, a, err, symmetrize, axis, bound, mac, add):
    """one FOR_IJK sweep exactly as written: cells in loop order, each seeing what the cells before it wrote.  a: [z][y][x] plane"""
    sx, sy, sz = dims
    size = dims[axis]
    s = size + (1 if mac else 0)
    for k in range(sz):
        for j in range(sy):
            for i in range(sx):
                idx, mdx = [i, j, k], [i, j, k]
                mdx[axis] = s - 1 - idx[axis]
                if mac and mdx[axis] >= size:
                    continue
                if bound > 0 and (not _in_bounds(dims, idx, bound) or not _in_bounds(dims, mdx, bound)):
                    continue
                I, Mi = (k, j, i), (mdx[2], mdx[1], mdx[0])
                if mac and mdx[axis] == idx[axis]:
                    if err is not None:
                        err[I] = f32(f64(err[I]) + abs(f64(a[I])))
                    if symmetrize:
                        a[I] = 0
                    continue
                if mac:
                    e = abs(f64(a[I]) - (f64(a[Mi]) * -1.))
                else:
                    e = f64(abs(f32(a[I] - a[Mi])))
                if err is not None:
                    err[I] = f32(f64(err[I]) + e) if add else f32(e)
                if symmetrize and idx[axis] < s // 2:
                    a[I] = -a[Mi] if mac else a[Mi]


def _sym_sweep_two_pass(dims, a, err, symmetrize, axis, bound, mac, add, cnt=None):
    """the restatement the kernels run: pass 0 the cells below the middle (and the MAC centre line), which read mirrors nothing writes;
    pass 1 the others, which read what pass 0 left.  Within a pass no cell reads what the pass writes, so it is written vectorised."""
    sx, sy, sz = dims
    size = dims[axis]
    s = size + (1 if mac else 0)
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    me = (i, j, k)[axis]
    mir = s - 1 - me
    valid = mir < size
    m3 = [i, j, k]
    m3[axis] = np.where(valid, mir, 0)
    if bound > 0:
        def inb(p):
            ok = (p[0] >= bound) & (p[1] >= bound) & (p[0] < sx - bound) & (p[1] < sy - bound)
            return ok & (((p[2] >= bound) & (p[2] < sz - bound)) if sz > 1 else (p[2] == 0))
        valid = valid & inb((i, j, k)) & inb(m3)
    centre = (mir == me) if mac else np.zeros_like(valid)
    first = centre | (me < s // 2)
    for ps in (0, 1):
        sel = valid & (first == (ps == 0))
        am = a[m3[2], m3[1], m3[0]]
        if mac:
            e = np.where(centre, np.abs(a.astype(f64)), np.abs(a.astype(f64) - (am.astype(f64) * -1.)))
        else:
            e = np.abs((a - am).astype(f32)).astype(f64)
        if err is not None:
            err[sel] = ((err.astype(f64) + e) if add else e).astype(f32)[sel]
        if symmetrize:
            new = np.where(centre, f32(0), -am if mac else am).astype(f32)
            wr = sel & (centre | (me < s // 2))
            a[wr] = new[wr]
        if cnt is not None:
            cnt["sym_pass%d" % ps] = cnt.get("sym_pass%d" % ps, 0) + int(sel.sum())
            cnt["sym_centre"] = cnt.get("sym_centre", 0) + int((sel & centre).sum())
            cnt["sym_skipped"] = cnt.get("sym_skipped", 0) + int((~valid).sum())


def check_symmetry(dims, a, with_err=True, symmetrize=False, axis=0, bound=0, disable=0, literal=False, cnt=None):
    """a: [z][y][x] (checkSymmetry) or [z][y][x][3] (checkSymmetryVec3) -> (a, err); err starts from NaN for the scalar form (every
    pair that is not skipped writes it) and from 0 for the MAC form (err->setConst(0))"""
    a = a.copy()
    mac = a.ndim == 4
    sweep = _sym_sweep_literal if literal else _sym_sweep_two_pass
    kw = {} if literal else {"cnt": cnt}
    if not mac:
        err = np.full(a.shape, np.nan, f32) if with_err else None
        sweep(dims, a, err, symmetrize, axis, bound, False, False, **kw)
        return a, err
    err = np.zeros(a.shape[:3], f32) if with_err else None
    for q in range(3):
        if disable >> q & 1:
            continue
        comp = (axis + q) % 3
        plane = np.ascontiguousarray(a[..., comp])
        sweep(dims, plane, err, symmetrize, axis, bound, q == 0, True, **kw)
        a[..., comp] = plane
    return a, err


def sym_input(shape, vec):
    sx, sy, sz = SYM_SHAPES[shape]
    r = np.random.default_rng(_seed("sym", shape, vec))
    return r.uniform(-2, 2, (sz, sy, sx) + ((3,) if vec else ())).astype(f32)


def init_grid_with_pos(dims):
    sx, sy, sz = dims
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return pd_norm3(np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(f32)).reshape(sz, sy, sx)


# ---- setNoisePdata* and addTestParts ---------------------------------------------------------------------------------------------
NOISE_N = 5000
NOISE_DIMS = (16, 12, 10)
NOISE_SCALE = {"real": 2.5, "int": 40.0, "vec3": 2.5}      # the int form truncates: a scale that leaves more than three values


def noise_positions():
    """positions inside the domain, on cell faces and centres, negative, and far outside the 128-cell tile period"""
    r = np.random.default_rng(_seed("noisepos"))
    p = r.uniform(0, 1, (NOISE_N, 3)) * np.array(NOISE_DIMS)
    p[:500] = np.floor(p[:500])                       # cell faces
    p[500:1000] = np.floor(p[500:1000]) + 0.5         # cell centres
    p[1000:1500] = r.uniform(-300, -1, (500, 3))
    p[1500:2000] = r.uniform(130, 2000, (500, 3))
    return p.astype(f32)


ADDPARTS = {"empty": (0, 5), "populated": (41, 7), "none": (12, 0)}
ADDPARTS_DIMS = (8, 7, 6)
PNEW = 1


def addparts_inputs(case):
    n0, num = ADDPARTS[case]
    r = np.random.default_rng(_seed("addparts", case))
    sx, sy, sz = ADDPARTS_DIMS
    return dict(n0=n0, num=num, pos=(r.uniform(0.5, 5, (n0, 3))).astype(f32), flags=r.integers(0, 4, n0).astype(i32),
                real=r.uniform(-1, 1, n0).astype(f32), vec=r.uniform(-1, 1, (n0, 3)).astype(f32), ints=r.integers(-9, 9, n0).astype(i32),
                plain=r.uniform(-1, 1, n0).astype(f32),
                src_real=r.uniform(1, 2, (sz, sy, sx)).astype(f32), src_mac=r.uniform(1, 2, (sz, sy, sx, 3)).astype(f32))


def add_test_parts(I):
    """no slot is deleted in these cases, so doCompress() moves nothing: PNEW cleared, `num` slots at the origin with PNEW; a channel
    with a source takes the source's value at the origin -- cell (0, 0, 0), every weight being (1, 0) there -- the others 0"""
    num = I["num"]
    z = np.zeros
    return dict(pos=np.concatenate([I["pos"], z((num, 3), f32)]), flags=np.concatenate([I["flags"] & ~PNEW, np.full(num, PNEW, i32)]),
                real=np.concatenate([I["real"], np.full(num, I["src_real"][0, 0, 0], f32)]),
                vec=np.concatenate([I["vec"], np.tile(I["src_mac"][0, 0, 0], (num, 1)).astype(f32)]),
                ints=np.concatenate([I["ints"], z(num, i32)]), plain=np.concatenate([I["plain"], z(num, f32)]))


def sym_digests(golden):
    """the symmetry part of the fixture: some eight hundred small arrays, kept as one table of SHA-256 digests (key -> digest)"""
    return dict(zip([str(k) for k in golden["symsha/keys"]], [str(v) for v in golden["symsha/shas"]]))


def sym_key(shape, axis, sym, bound, vec, dis, with_err):
    return "sym/%s/%d/%d/%d/%s%d/%d" % (shape, axis, int(sym), bound, "vec" if vec else "real", dis, int(with_err))


# ---- the loops of test_2005_symmAdv.py and test_2065_partIo.py: recorded reference runs (tools/record_grid4d.py), no model -----------
LOOP2005 = {"res": 12, "steps": 2}
LOOP2065 = {"res": 16, "fixedSeed": 265, "every": 16}       # final positions are kept for every 16th particle (and as a digest)
