"""numpy statement of the smoke data-generation plugins (include/open/manta_hip_datagen.h) and the cases of their tests.

Grids are float32 arrays [z][y][x] (one component) or [z][y][x][3]; every function rounds where the reference rounds (its Real is
float; a literal such as 2.0, 0.5 or 1. makes an expression double until the next store into a Real).  tools/record_datagen.py asserts
that these functions reproduce the reference's outputs before it writes tests/golden/datagen.npz; inputs come from the seeded
generators below and are never stored.
"""
import math
import os

import numpy as np

from reduce_model import fixed_order_sum          # the centre of mass: 1024 cells per block, at most 2048 blocks (its defaults)

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen.npz")
MAX_TAPS = 255


def same(a, b):
    """bit for bit, except that a NaN equals any NaN (the sign and payload of a generated NaN are the hardware's choice)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    u = "u%d" % a.dtype.itemsize
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


def differing(a, b):
    """how many elements are not the same in the sense of same()"""
    u = "u%d" % a.dtype.itemsize
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(u) != b.view(u)))).sum())


def dims_of(a):
    """(sx, sy, sz) of a grid array"""
    return a.shape[2], a.shape[1], a.shape[0]


# ---- blur -------------------------------------------------------------------------------------------------------------------------
def weights(sigma):
    """GaussianKernelCreator::setGaussianSigma, initplugins.cpp:535-557: (mDim, the mDim weights); not normalised"""
    sigma = f32(sigma)
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be positive")
    mDim = int(2.0 * 3.0 * float(sigma) + 1.0)
    if mDim < 3:
        mDim = 3
    if mDim % 2 == 0:
        mDim += 1
    s2 = sigma * sigma
    c = mDim // 2
    m = f32(1.0 / (math.sqrt(2.0 * math.pi) * float(sigma)))
    w = np.zeros(mDim, f32)
    for i in range((mDim + 1) // 2):
        v = f32(float(m) * math.exp(-(1.0 * i * i) / (2.0 * float(s2))))
        w[c + i] = v
        w[c - i] = v
    return mDim, w


def blur_pass(src, w, axis):
    """one pass along grid axis 0 x, 1 y, 2 z: acc = 0; acc += w[d] * src[clamp(pos - (d - mDim/2))] for d = 0 .. mDim-1, product and
    sum rounded separately in fp32"""
    ax = 2 - axis                         # arrays are [z][y][x](,[3])
    n, c = len(w), len(w) // 2
    pos = np.arange(src.shape[ax])
    acc = np.zeros_like(src)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(n):
            tap = np.take(src, np.clip(pos - (d - c), 0, src.shape[ax] - 1), axis=ax)
            acc = acc + w[d] * tap
    return acc


def blur(src, sigma):
    """blurRealGrid / blurMacGrid: (the blurred grid, mDim); x, y and, on a 3-D grid, z"""
    mDim, w = weights(sigma)
    g = blur_pass(np.ascontiguousarray(src, f32), w, 0)
    g = blur_pass(g, w, 1)
    if src.shape[0] > 1:
        g = blur_pass(g, w, 2)
    return g, mDim


# ---- centre of mass ---------------------------------------------------------------------------------------------------------------
def com_terms(density):
    """the reference's four terms per cell, in cell order: density * (i + 0.5f), * (j + 0.5f), * (k + 0.5f) as fp32 products, density"""
    sz, sy, sx = density.shape
    d = np.ascontiguousarray(density, f32)
    k, j, i = np.meshgrid(np.arange(sz, dtype=f32) + f32(0.5), np.arange(sy, dtype=f32) + f32(0.5), np.arange(sx, dtype=f32) + f32(0.5),
                          indexing="ij")
    return [(d * i).ravel(), (d * j).ravel(), (d * k).ravel(), d.ravel()]


def center_of_mass(density):
    """the contract: fp32 terms, fp64 sums in the fixed order, w rounded to fp32 for the `> 1e-6f` test, fp64 quotients rounded once"""
    s = [fixed_order_sum(t) for t in com_terms(density)]
    if f32(s[3]) > f32(1e-6):
        return np.array([f32(s[q] / s[3]) for q in range(3)], f32)
    return np.array([f32(s[q]) for q in range(3)], f32)


def center_of_mass_serial(density):
    """the reference itself, initplugins.cpp:337-348: serial fp32 sums, k outer and i inner, an fp32 quotient"""
    t = com_terms(density)
    s = [f32(0)] * 4
    for q in range(4):
        a = f32(0)
        for v in t[q]:
            a = f32(a + v)
        s[q] = a
    if s[3] > f32(1e-6):
        return np.array([s[q] / s[3] for q in range(3)], f32)
    return np.array(s[:3], f32)


def com_bound(density, c_ref):
    """per component, the forward error bound of the reference's two fp32 sums and its quotient:
    ((2 gamma(n-1) sum|t_c| / |sum t_c|) + 4u) |c|, u = 2^-24, gamma(k) = k u / (1 - k u)"""
    u = 2.0 ** -24
    t = com_terms(density)
    n = t[0].size
    gamma = (n - 1) * u / (1.0 - (n - 1) * u)
    out = []
    for q in range(3):
        sa, ss = math.fsum(abs(float(v)) for v in t[q]), abs(math.fsum(float(v) for v in t[q]))
        ratio = sa / ss if ss > 0 else 1.0
        out.append((2.0 * gamma * ratio + 4.0 * u) * abs(float(c_ref[q])))
    return out


# ---- projection -------------------------------------------------------------------------------------------------------------------
def light(val):
    """gridPrecompLight, simpleimage.cpp:206-215: dot((1, 1, 1), normalize(getGradient(val) * -1.)) in every cell"""
    sz, sy, sx = val.shape
    K, J, I = np.meshgrid(np.arange(sz), np.clip(np.arange(sy), 1, sy - 2), np.clip(np.arange(sx), 1, sx - 2), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gx = -(val[K, J, I + 1] - val[K, J, I - 1])
        gy = -(val[K, J + 1, I] - val[K, J - 1, I])
        if sz > 1:
            KK = np.clip(K, 1, sz - 2)
            gz = -(val[KK + 1, J, I] - val[KK - 1, J, I])
        else:
            gz = np.full(val.shape, -0.0, f32)
        l = (gx * gx + gy * gy) + gz * gz
        eps2 = f32(1e-6) * f32(1e-6)
        near1 = np.abs(l.astype(f64) - 1.) < float(eps2)
        big = ~near1 & (l > eps2)
        fac = (1. / np.sqrt(l).astype(f64)).astype(f32)
        zero = np.zeros_like(l)
        gx, gy, gz = (np.where(near1, g, np.where(big, g * fac, zero)) for g in (gx, gy, gz))
        return (gx + gy) + gz


def _march(src, lit, surf):
    """shadeCell (simpleimage.cpp:218-244) over src[depth][a][b] in order of depth: the [a][b][3] pixels"""
    depth = src.shape[0]
    depthInv = f32(1. / float(f32(depth)))
    dst = np.zeros(src.shape[1:] + (3,), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(depth):
            s = src[m]
            if surf:
                t = f32(m) * depthInv
                tint = f32(float(f32(0.9)) * (float(t) * 0.7 + 0.3))
                a1 = 1. - s.astype(f64)
                for c, dif in enumerate((tint, tint, f32(0.9))):
                    col = f32(0.1) + dif * lit[m]
                    keep = (a1 * dst[..., c].astype(f64)).astype(f32)
                    dst[..., c] = keep + s * col
            else:
                p = depthInv * s
                for c in range(3):
                    dst[..., c] = dst[..., c] + p
    return dst


def project(val, shadeMode=0, scale=1., views=7):
    """projectImg + writePpm's bytes: the (h, w, 3) uint8 image in file row order (top row first)"""
    val = np.ascontiguousarray(val, f32)
    sz, sy, sx = val.shape
    is3d = sz > 1
    w, h = (sx + sz + sx if is3d else sx), max(sx, sy, sz)
    surf = shadeMode == 1
    lit = light(val) if surf else None
    img = np.zeros((h, w, 3), f32)
    if views & 1:
        img[:sy, :sx] = _march(val, lit, surf)                                                        # [k][j][i] -> pixel (i, j)
    if is3d and views & 2:
        img[:sy, sx:sx + sz] = _march(val.transpose(2, 1, 0), lit.transpose(2, 1, 0) if surf else None, surf)    # [i][j][k] -> (sx + k, j)
    if is3d and views & 4:
        img[:sz, sx + sz:] = _march(val.transpose(1, 0, 2), lit.transpose(1, 0, 2) if surf else None, surf)      # [j][k][i] -> (sx + sz + i, k)
    f = f32(1. / float(f32(scale)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = img / f
        v = np.where(v < 0, f32(0), np.where(v > 1, f32(1), v))
        b = (255. * v.astype(f64)).astype(np.uint8)
    return np.ascontiguousarray(b[::-1])


def ppm_bytes(img):
    h, w, _ = img.shape
    return ("P6\n%d %d\n255\n" % (w, h)).encode() + img.tobytes()


def read_ppm(path):
    raw = open(path, "rb").read()
    head, rest = raw.split(b"\n255\n", 1)
    magic, size = head.split(b"\n")
    assert magic == b"P6"
    w, h = (int(v) for v in size.split())
    assert len(rest) == w * h * 3
    return np.frombuffer(rest, np.uint8).reshape(h, w, 3).copy()


# ---- Laplacian and curvature --------------------------------------------------------------------------------------------------------
def _inner(a):
    sz = a.shape[0]
    return (slice(1, sz - 1) if sz > 1 else slice(0, 1), slice(1, a.shape[1] - 1), slice(1, a.shape[2] - 1))


def _sh(a, di, dj, dk):
    """a(i + di, j + dj, k + dk) on the interior"""
    sz, sy, sx = a.shape
    zs = slice(1 + dk, sz - 1 + dk) if sz > 1 else slice(0, 1)
    return a[zs, 1 + dj:sy - 1 + dj, 1 + di:sx - 1 + di]


def laplacian(g, out):
    """LaplaceOp, commonkernels.h:75-80, into a copy of out (the border keeps its values)"""
    g = np.ascontiguousarray(g, f32)
    out = np.array(out, f32)
    D = lambda di, dj, dk: _sh(g, di, dj, dk).astype(f64)
    c2 = 2.0 * D(0, 0, 0)
    l = ((D(1, 0, 0) - c2) + D(-1, 0, 0)).astype(f32)
    l = (l.astype(f64) + ((D(0, 1, 0) - c2) + D(0, -1, 0))).astype(f32)
    if g.shape[0] > 1:
        l = (l.astype(f64) + ((D(0, 0, 1) - c2) + D(0, 0, -1))).astype(f32)
    out[_inner(g)] = l
    return out


def curvature_parts(g, h=1.0):
    """CurvatureOp, commonkernels.h:83-100 up to the last line: (the numerator as stored in curv, max(denom, 1e-6f)) on the interior"""
    g = np.ascontiguousarray(g, f32)
    S = lambda di, dj, dk: _sh(g, di, dj, dk)
    D = lambda di, dj, dk: _sh(g, di, dj, dk).astype(f64)
    oh = float(f32(1.0 / float(f32(h))))
    c2 = 2.0 * D(0, 0, 0)
    first = lambda a, b: ((0.5 * (a - b).astype(f64)) * oh).astype(f32)
    second = lambda a, b: ((((a - c2) + b) * oh) * oh).astype(f32)
    mixed = lambda a, b, c, d: (((0.25 * (((a + b) - c) - d).astype(f64)) * oh) * oh).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = first(S(1, 0, 0), S(-1, 0, 0)), first(S(0, 1, 0), S(0, -1, 0))
        xx, yy = second(D(1, 0, 0), D(-1, 0, 0)), second(D(0, 1, 0), D(0, -1, 0))
        xy = mixed(S(1, 1, 0), S(-1, -1, 0), S(-1, 1, 0), S(1, -1, 0))
        x2, y2 = x * x, y * y
        cv = ((x2 * yy + y2 * xx).astype(f64) - ((2.0 * x.astype(f64)) * y.astype(f64)) * xy.astype(f64)).astype(f32)
        denom = x2 + y2
        if g.shape[0] > 1:
            z = first(S(0, 0, 1), S(0, 0, -1))
            zz = second(D(0, 0, 1), D(0, 0, -1))
            xz = mixed(S(1, 0, 1), S(-1, 0, -1), S(-1, 0, 1), S(1, 0, -1))
            yz = mixed(S(0, 1, 1), S(0, -1, -1), S(0, 1, -1), S(0, -1, 1))
            z2 = z * z
            n1 = ((x2 * zz + z2 * xx) + y2 * zz) + z2 * yy
            mx = (x * z) * xz + (y * z) * yz
            cv = (cv.astype(f64) + (n1.astype(f64) - 2.0 * mx.astype(f64))).astype(f32)
            denom = denom + z2
        dm = np.where(denom < f32(1e-6), f32(1e-6), denom)
    return cv, dm


def curvature(g, out, h=1.0):
    """CurvatureOp into a copy of out; the fp64 pow is the C library's (math.pow), as in the reference"""
    out = np.array(out, f32)
    cv, dm = curvature_parts(g, h)
    pw = np.array([math.pow(float(v), 1.5) for v in dm.ravel()], f64).reshape(dm.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        out[_inner(np.asarray(g))] = (cv.astype(f64) / pw).astype(f32)
    return out


def ulp_of(ref):
    """the fp32 spacing at each reference value (subnormal spacing included)"""
    a = np.abs(np.asarray(ref, f32))
    with np.errstate(over="ignore"):
        return (np.nextafter(a, f32(np.inf)) - a).astype(f64)


def within_one_ulp(got, ref):
    """(every cell within 1 fp32 ulp of the reference value, how many cells are not bit-identical)"""
    got, ref = np.asarray(got, f32), np.asarray(ref, f32)
    nd = differing(got, ref)
    na, nb = np.isnan(got), np.isnan(ref)
    if (na != nb).any():
        return False, nd
    ok = ~na
    inf = np.isinf(ref) & ok
    if (got[inf] != ref[inf]).any():
        return False, nd
    ok &= ~inf
    return bool((np.abs(got[ok].astype(f64) - ref[ok].astype(f64)) <= ulp_of(ref[ok])).all()), nd


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SENTINEL = f32(-7.25)
WEIGHT_SIGMAS = ((0.1, 3), (0.25, 3), (0.5, 5), (0.564, 5), (1.128, 7), (3.0, 19))
WEIGHT_DIMS = (9, 8, 1)
# name -> ((sx, sy, sz), sigma)
BLUR_CASES = {
    "row67": ((67, 5, 3), 1.128),       # a row over one wavefront, with a tail
    "wide": ((5, 4, 3), 3.0),           # the kernel is wider than every axis: the clamp acts on both sides of every tap
    "thin2d": ((3, 50, 1), 0.564),      # 2-D: no z pass
    "flat2d": ((33, 18, 1), 1.128),
    "deep": ((9, 7, 35), 0.564),
    "row64": ((64, 3, 3), 0.5),
    "row65": ((65, 3, 3), 0.25),
}
BLUR_SPECIAL = ((9, 7, 5), 0.564)        # one NaN, one +inf and one -inf cell


def _rng(*key):
    return np.random.default_rng([20261020] + [int(k) for k in key])


def grid_noise(dims, seed, lo=-1.0, hi=1.0, ncomp=1):
    sx, sy, sz = dims
    shape = (sz, sy, sx) if ncomp == 1 else (sz, sy, sx, ncomp)
    return _rng(seed, sx, sy, sz, ncomp).uniform(lo, hi, shape).astype(f32)


def blur_input(name, ncomp):
    if name == "special":
        a = grid_noise(BLUR_SPECIAL[0], 5, ncomp=ncomp)
        for q, (cell, v) in enumerate((((2, 3, 4), np.nan), ((0, 0, 0), np.inf), ((4, 6, 8), -np.inf))):
            if ncomp == 1:
                a[cell] = v
            else:
                a[cell + (q,)] = v
        return a
    if name[0] == "w" and name[1:].isdigit():
        return grid_noise(WEIGHT_DIMS, 3, ncomp=ncomp)
    return grid_noise(BLUR_CASES[name][0], 4, ncomp=ncomp)


def blur_cases():
    """(name, dims, sigma) of every recorded blur"""
    out = [("w%d" % q, WEIGHT_DIMS, s) for q, (s, _) in enumerate(WEIGHT_SIGMAS)]
    out += [(n, d, s) for n, (d, s) in BLUR_CASES.items()]
    out.append(("special", BLUR_SPECIAL[0], BLUR_SPECIAL[1]))
    return out


COM_CASES = ("exact3d", "exact2d", "pos3d", "mixed3d", "pos2d", "mixed2d", "zero", "tiny")
COM_EXACT = ("exact3d", "exact2d", "zero", "tiny")      # every fp32 partial sum of the reference is exact: bit-identical


def com_input(name):
    if name in ("exact3d", "exact2d"):
        sx, sy, sz = (12, 10, 8) if name == "exact3d" else (16, 16, 1)
        return (_rng(6, sx, sy, sz).integers(0, 257, (sz, sy, sx)) / 64.0).astype(f32)       # multiples of 2^-6 in [0, 4]
    if name in ("pos3d", "mixed3d", "pos2d", "mixed2d"):
        dims = (33, 31, 29) if name.endswith("3d") else (37, 29, 1)
        return grid_noise(dims, 7, 0.0 if name.startswith("pos") else -0.25, 1.0)
    a = np.zeros((1, 5, 6), f32)
    if name == "tiny":                   # w = 3 * 2^-22 = 7.15e-7, in (0, 1e-6]: the undivided branch
        a[0, 3, 2] = f32(2.0 ** -21)
        a[0, 1, 4] = f32(2.0 ** -22)
    return a


PROJECT_DIMS = ((7, 5, 4), (5, 9, 6), (4, 6, 11), (70, 5, 3), (12, 9, 1))
PROJECT_MODES = (0, 1, 3)
PROJECT_SCALES = (1.0, 4.0, 0.5)


def project_input(dims):
    return grid_noise(dims, 8, -0.3, 1.6)       # values below 0 and above 1: the clamp and the truncation both act


def project_const():
    return np.full((4, 5, 7), 0.5, f32)          # mode 1 on a constant grid: the zero-vector branch of normalize


def project_key(dims, mode, scale):
    return "project/%dx%dx%d/m%d/s%g" % (dims + (mode, scale))


STENCIL_DIMS = ((7, 5, 4), (67, 5, 3), (33, 31, 29), (12, 9, 1))
STENCIL_BIG = (33, 31, 29)


def stencil_input(kind, dims):
    sx, sy, sz = dims
    if kind == "const":
        return np.full((sz, sy, sx), 0.75, f32)
    if kind == "noise":
        return grid_noise(dims, 9, -2.0, 2.0)
    k, j, i = np.meshgrid(np.arange(sz, dtype=f64), np.arange(sy, dtype=f64), np.arange(sx, dtype=f64), indexing="ij")
    c = ((sx - 1) * 0.5 + 0.3, (sy - 1) * 0.5 - 0.2, (sz - 1) * 0.5 + 0.1 if sz > 1 else 0.0)
    r = 0.3 * min(sx, sy, sz if sz > 1 else sx)
    return (np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - r).astype(f32)      # a sphere level set


def stencil_cases():
    """(key, kind, dims, h) of every recorded curvature; h is None for the recorded Laplacians"""
    out = []
    for dims in STENCIL_DIMS:
        tag = "%dx%dx%d" % dims
        if dims == STENCIL_BIG:          # the large shape: one h per input keeps the fixture small
            combos = (("sphere", 1.0), ("noise", 0.5), ("const", 1.0))
            laps = ("noise",)
        else:
            combos = tuple((kind, h) for kind in ("sphere", "const", "noise") for h in (1.0, 0.5))
            laps = ("sphere", "noise")
        out += [("curv/%s/%s/h%g" % (tag, kind, h), kind, dims, h) for kind, h in combos]
        out += [("lap/%s/%s" % (tag, kind), kind, dims, None) for kind in laps]
    return out


# ---- the two recorded loops ---------------------------------------------------------------------------------------------------------
ST_LOOP = dict(res=20, steps=5)      # scenes/surfaceTension.py without the mesh line
# The simMode == 1 loop of tensorflow/example3_resnet/manta_genSimData2.py in 3-D with re-centring on; the script's random draws are
# these constants (all but the noise parameters and the gravities exactly representable in fp32).  src: fine centre, coarse centre and
# sphere scale of the two density sources (the second is the inflow); srcr: fine and coarse radius; noise: posScale, valOffset and the
# fine timeAnim; ini: fine centre, radius and velocity, coarse centre, radius and velocity of the two initial-velocity spheres; buoy: the
# y gravity of the fine and of the coarse solver.
DG_LOOP = dict(
    res=16, steps=6, warm=3, scaleFactor=2, resetN=2, seeds=(1234, 777),
    src=((19.25, 17.5, 13.5, 9.625, 8.75, 6.75, 1.0, 0.96875, 1.03125), (13.0, 9.0, 17.5, 6.5, 4.5, 8.75, 1.03125, 1.0, 0.96875)),
    srcr=((4.5, 2.25), (4.0, 2.0)),
    noise=((4.75, 0.1875, 0.3), (3.5, 0.375, 0.3)),
    ini=((12.5, 20.25, 14.0, 3.25, 0.75, -0.5, 0.375, 6.25, 10.125, 7.0, 1.625, 0.375, -0.25, 0.1875),
         (21.0, 11.5, 18.25, 2.75, -0.625, 0.5, -0.25, 10.5, 5.75, 9.125, 1.375, -0.3125, 0.25, -0.125)),
    buoy=(-0.0005, -0.00025))
