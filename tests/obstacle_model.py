"""float32 numpy restatement of the fill-fraction obstacle plugins (include/manta_hip_obstacles.h), for tests.

Grids are numpy arrays in the package's layout: flags / Real grids [sz, sy, sx], MAC grids SoA [3, sz, sy, sx].  Every step keeps
the reference's float / double promotion points (Real = float, double literals promote), so the model is bit-exact.

  update_fractions       calcFraction + KnUpdateFractions (bnd=1) after setConst(0), plugin/initplugins.cpp:351-440,
                         serial i, j, k sweep order (one OpenMP thread)
  set_obstacle_flags     KnUpdateFlagsObs (bnd=boundaryWidth), plugin/initplugins.cpp:442-474
  set_wall_bcs_frac      KnSetWallBcsFrac + vel.swap(tmpvel), plugin/extforces.cpp:240-335; normalize, util/vectorbase.h:421-433;
                         getAtMACX/Y/Z, grid.h:473-505
  set_inflow_bcs         KnSetInflow / setInflowBcs, plugin/extforces.cpp:163-182
  add_noise              KnAddNoise, plugin/initplugins.cpp:45-51; WaveletNoiseField::evaluate / WNoise, noisefield.h:118-137, 313-336
"""
import numpy as np

f32, f64 = np.float32, np.float64
FLUID, OBSTACLE, EMPTY, INFLOW, OUTFLOW, OPEN = 1, 2, 4, 8, 16, 32
OPENISH = INFLOW | OUTFLOW | OPEN


def _ijk(shape):
    return np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")


def kernel_range(shape, b, k, j, i):
    """cells a KERNEL(bnd=b) visits (kernel.cpp:21-30: the k loop runs [b, sz-b) when sz-b > 1 in 3-D, else plane 0)"""
    sz, sy, sx = shape
    is3d = sz > 1
    m = (i >= b) & (i < sx - b) & (j >= b) & (j < sy - b)
    maxZ, minZ = (sz - b, b) if is3d else (1, 0)
    return m & ((k >= minZ) & (k < maxZ) if maxZ > 1 else (k == 0))


def calc_fraction(phi1, phi2, thr):
    """calcFraction, initplugins.cpp:356-371"""
    phi1, phi2 = phi1.astype(f32), phi2.astype(f32)
    sw = phi2 < phi1
    lo, hi = np.where(sw, phi2, phi1), np.where(sw, phi1, phi2)
    denom = (lo - hi).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (lo / denom).astype(f32)
    frac = (f64(1.) - q.astype(f64)).astype(f32)
    frac = np.where(frac < f32(thr), f32(0), frac)
    frac = np.where(frac < f32(1), frac, f32(1))
    out = np.where(denom.astype(f64) > -1e-04, f32(0.5), frac)
    out = np.where((phi1 < 0) & (phi2 < 0), f32(0), out)
    out = np.where((phi1 > 0) & (phi2 > 0), f32(1), out)
    return out.astype(f32)


def _shift(a, axis, d, fill=0):
    """b[p] = a[p - d e_axis] where that index exists, else fill"""
    b = np.full_like(a, fill)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if d > 0:
        src[axis], dst[axis] = slice(0, a.shape[axis] - d), slice(d, None)
    else:
        src[axis], dst[axis] = slice(-d, None), slice(0, a.shape[axis] + d)
    b[tuple(dst)] = a[tuple(src)]
    return b


def update_fractions(flags, phi, boundaryWidth=0, fracThreshold=0.01):
    """fractions after updateFractions(flags, phi, fractions, boundaryWidth, fracThreshold)"""
    shape = flags.shape
    is3d = shape[0] > 1
    k, j, i = _ijk(shape)
    w = int(boundaryWidth)
    sz, sy, sx = shape
    phi = phi.astype(f32)
    fr = np.zeros((3,) + shape, f32)
    inr = kernel_range(shape, 1, k, j, i)
    # own result of the cells in range
    px, py = _shift(phi, 2, 1), _shift(phi, 1, 1)
    own = [calc_fraction(phi, px, fracThreshold), calc_fraction(phi, py, fracThreshold)]
    own.append(calc_fraction(phi, _shift(phi, 0, 1), fracThreshold) if is3d else np.zeros(shape, f32))
    notobs = ~(phi < 0)
    fx, fy = _shift(flags, 2, 1), _shift(flags, 1, 1)
    mins = ((i <= w + 1) & ((fx & OPENISH) != 0)) | ((j <= w + 1) & ((fy & OPENISH) != 0))
    if is3d:
        mins |= (k <= w + 1) & ((_shift(flags, 0, 1) & OPENISH) != 0)
    one_in = inr & notobs & mins
    # cells outside the range: the "max" rules of their -x / -y / -z neighbour
    op = (flags & OPENISH) != 0
    nx = _shift(inr, 2, 1, False) & ~(_shift(phi, 2, 1) < 0) & (i - 1 >= sx - w - 2)
    ny = _shift(inr, 1, 1, False) & ~(_shift(phi, 1, 1) < 0) & (j - 1 >= sy - w - 2)
    one_out = nx | ny
    if is3d:
        one_out |= _shift(inr, 0, 1, False) & ~(_shift(phi, 0, 1) < 0) & (j >= sz - w - 2)
    one_out &= ~inr & op
    for c in range(3):
        fr[c] = np.where(inr, own[c], f32(0))
    one = one_in | one_out
    for c in range(3 if is3d else 2):
        fr[c][one] = f32(1)
    return fr


def set_obstacle_flags(flags, phi, fractions=None, phiOut=None, phiIn=None, boundaryWidth=1):
    """flags after setObstacleFlags(flags, phi, fractions, phiOut, phiIn, boundaryWidth)"""
    shape = flags.shape
    is3d = shape[0] > 1
    k, j, i = _ijk(shape)
    inr = kernel_range(shape, int(boundaryWidth), k, j, i)
    if fractions is not None:
        fr = fractions.astype(f32)
        terms = [fr[0], _shift(fr[0], 2, -1), fr[1], _shift(fr[1], 1, -1)]
        if is3d:
            terms += [fr[2], _shift(fr[2], 0, -1)]
        f = np.zeros(shape, f32)
        for t in terms:
            f = (f + t).astype(f32)
        isObs = f == 0
    else:
        isObs = phi < 0
    isOut = (phiOut < 0) if phiOut is not None else np.zeros(shape, bool)
    isIn = (phiIn < 0) if phiIn is not None else np.zeros(shape, bool)
    v = np.where(isObs, OBSTACLE, np.where(isIn, FLUID | INFLOW, np.where(isOut, EMPTY | OUTFLOW, EMPTY))).astype(np.int32)
    return np.where(inr, v, flags).astype(np.int32)


def _avg(a, b):
    return ((a + b).astype(f32).astype(f64) * .5).astype(f32)


def _normalize(x, y, z):
    l = ((x * x + y * y).astype(f32) + z * z).astype(f32)
    eps2 = f32(1e-6) * f32(1e-6)
    keep = np.abs(l.astype(f64) - 1.) < f64(eps2)
    scale = l > eps2
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (1. / np.sqrt(l).astype(f32).astype(f64)).astype(f32)
    out = []
    for c in (x, y, z):
        out.append(np.where(keep, c, np.where(scale, (c * s).astype(f32), f32(0))).astype(f32))
    return out


def _unproject(d, v, comp):
    dt = ((d[0] * v[0]).astype(f32) + (d[1] * v[1]).astype(f32)).astype(f32)
    dt = (dt + (d[2] * v[2]).astype(f32)).astype(f32)
    return (v[comp] - (dt * d[comp]).astype(f32)).astype(f32)


def _q4(a, b, c, d):
    return ((((a + b).astype(f32) + c).astype(f32) + d).astype(f32) * f32(0.25)).astype(f32)


def set_wall_bcs_frac(flags, vel, phi):
    """vel after setWallBcs(flags, vel, fractions=..., phiObs=phi)"""
    shape = flags.shape
    sz, sy, sx = shape
    is3d = sz > 1
    n = flags.size
    Y, Z = sx, (sx * sy if is3d else 0)
    fl = flags.reshape(-1)
    P = phi.astype(f32).reshape(-1)
    V = vel.astype(f32).reshape(3, -1)
    out = V.copy()
    k, j, i = (a.reshape(-1) for a in _ijk(shape))
    inb = (i >= 1) & (j >= 1) & (i < sx - 1) & (j < sy - 1) & (((k >= 1) & (k < sz - 1)) if is3d else (k == 0))
    cur = ((fl & (FLUID | OBSTACLE)) != 0) & inb
    curObs = (fl & OBSTACLE) != 0
    idx = np.nonzero(cur)[0]
    ob = lambda q: (fl[q] & OBSTACLE) != 0

    # x faces
    q = idx[curObs[idx] | ob(idx - 1)]
    if q.size:
        t1 = _avg(P[q], P[q - 1])
        phi1, phi2 = _avg(t1, _avg(P[q + Y], P[q - 1 + Y])), _avg(t1, _avg(P[q - Y], P[q - 1 - Y]))
        d = [(P[q] - P[q - 1]).astype(f32), (phi1 - phi2).astype(f32), np.zeros(q.size, f32)]
        if is3d:
            d[2] = (_avg(t1, _avg(P[q + Z], P[q - 1 + Z])) - _avg(t1, _avg(P[q - Z], P[q - 1 - Z]))).astype(f32)
        d = _normalize(*d)
        v = [V[0][q], _q4(V[1][q], V[1][q - 1], V[1][q + Y], V[1][q + Y - 1]), np.zeros(q.size, f32)]
        if is3d:
            v[2] = _q4(V[2][q], V[2][q - 1], V[2][q + Z], V[2][q + Z - 1])
        out[0][q] = _unproject(d, v, 0)
    # y faces
    q = idx[curObs[idx] | ob(idx - Y)]
    if q.size:
        t1 = _avg(P[q], P[q - Y])
        phi1, phi2 = _avg(t1, _avg(P[q + 1], P[q + 1 - Y])), _avg(t1, _avg(P[q - 1], P[q - 1 - Y]))
        d = [(phi1 - phi2).astype(f32), (P[q] - P[q - Y]).astype(f32), np.zeros(q.size, f32)]
        if is3d:
            d[2] = (_avg(t1, _avg(P[q + Z], P[q - Y + Z])) - _avg(t1, _avg(P[q - Z], P[q - Y - Z]))).astype(f32)
        d = _normalize(*d)
        v = [_q4(V[0][q], V[0][q - Y], V[0][q + 1], V[0][q + 1 - Y]), V[1][q], np.zeros(q.size, f32)]
        if is3d:
            v[2] = _q4(V[2][q], V[2][q - Y], V[2][q + Z], V[2][q + Z - Y])
        out[1][q] = _unproject(d, v, 1)
    # z faces
    if is3d:
        q = idx[curObs[idx] | ob(idx - Z)]
        if q.size:
            t1 = _avg(P[q], P[q - Z])
            dx = (_avg(t1, _avg(P[q + 1], P[q + 1 - Z])) - _avg(t1, _avg(P[q - 1], P[q - 1 - Z]))).astype(f32)
            dy = (_avg(t1, _avg(P[q + Y], P[q + Y - Z])) - _avg(t1, _avg(P[q - Y], P[q - Y - Z]))).astype(f32)
            d = _normalize(dx, dy, (P[q] - P[q - Z]).astype(f32))
            v = [_q4(V[0][q], V[0][q - Z], V[0][q + 1], V[0][q + 1 - Z]),
                 _q4(V[1][q], V[1][q - Z], V[1][q + Y], V[1][q + Y - Z]), V[2][q]]
            out[2][q] = _unproject(d, v, 2)
    return out.reshape((3,) + shape)


def set_inflow_bcs(vel, dir, value):
    """vel after setInflowBcs(vel, dir, value) (raises like the reference after applying the characters before a bad one)"""
    out = vel.astype(f32).copy()
    shape = out.shape[1:]
    k, j, i = _ijk(shape)
    pos, size = (i, j, k), (shape[2], shape[1], shape[0])
    val = [f32(v) for v in value]
    for ch in dir:
        if "x" <= ch <= "z":
            dim, p0 = ord(ch) - ord("x"), 0
        elif "X" <= ch <= "Z":
            dim = ord(ch) - ord("X")
            p0 = size[dim] - 1
        else:
            raise RuntimeError("invalid character in direction string. Only [xyzXYZ] allowed.")
        m = (pos[dim] == p0) | (pos[dim] == p0 + 1)
        for c in range(3):
            out[c][m] = val[c]
    return out


def noise_evaluate(tile, params, x, y, z):
    """WaveletNoiseField::evaluate(Vec3(x, y, z)) for float32 arrays x, y, z; params: the 20-float block of NoiseField._params()"""
    P = [f32(v) for v in params]
    pos = [np.asarray(a, f32) for a in (x, y, z)]
    pos = [(pos[c] * P[c]).astype(f32) for c in range(3)]
    pos = [(pos[c] + P[3 + c]).astype(f32) for c in range(3)]
    pos = [(pos[c] + P[6]).astype(f32) for c in range(3)]
    pos = [(pos[c] * P[7 + c]).astype(f32) for c in range(3)]
    pos = [(pos[c] + P[10 + c]).astype(f32) for c in range(3)]
    w, mid = [], []
    for c in range(3):
        pm = (pos[c] - f32(0.5)).astype(f32)
        m = np.ceil(pm).astype(np.int64)
        t = (m.astype(f32) - pm).astype(f32)
        w0 = ((t * t).astype(f32) * f32(0.5)).astype(f32)
        u = (f32(1) - t).astype(f32)
        w2 = ((u * u).astype(f32) * f32(0.5)).astype(f32)
        w1 = ((f32(1) - w0).astype(f32) - w2).astype(f32)
        w.append((w0, w1, w2))
        mid.append(m)
    data = tile[:128 ** 3]
    res = np.zeros(pos[0].shape, f32)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                wt = (f32(1) * w[0][dx + 1]).astype(f32)
                wt = (wt * w[1][dy + 1]).astype(f32)
                wt = (wt * w[2][dz + 1]).astype(f32)
                xc, yc, zc = (mid[0] + dx) & 127, (mid[1] + dy) & 127, (mid[2] + dz) & 127
                res = (res + (wt * data[(zc * 128 + yc) * 128 + xc]).astype(f32)).astype(f32)
    res = (res + P[13]).astype(f32)
    res = (res * P[14]).astype(f32)
    if P[15] != 0:
        res = np.where(res < P[16], P[16], res)
        res = np.where(res > P[17], P[17], res).astype(f32)
    return res


def add_noise(flags, density, tile, params, sdf=None, scale=1.0):
    """density after addNoise(flags, density, noise, sdf, scale)"""
    k, j, i = _ijk(flags.shape)
    m = (flags & FLUID) != 0
    if sdf is not None:
        m &= ~(sdf > 0)
    nv = noise_evaluate(tile, params, i[m].astype(f32), j[m].astype(f32), k[m].astype(f32))
    out = density.astype(f32).copy()
    out[m] = (out[m] + (nv * f32(scale)).astype(f32)).astype(f32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs (the golden file holds outputs only; these regenerate the inputs it was recorded from)
# ---------------------------------------------------------------------------------------------------------------------------
_SIDE = {"w": OBSTACLE, "i": INFLOW, "o": OUTFLOW, "p": OPEN}


def scene_inputs(dims, seed, sides="wwwwww", bw=0, fluid_frac=0.5, zero_frac=0.05):
    """flags + phiObs of a random obstacle scene: border layers of width bw+1 per side (sides: one of w/i/o/p per side in the
    order x, X, y, Y, z, Z, overwritten in that order as FlagGrid::initBoundaries does), random Fluid / Empty inside, a sphere
    levelset with noise and a few exact zeros"""
    sx, sy, sz = dims
    shape = (sz, sy, sx)
    is3d = sz > 1
    rng = np.random.RandomState(seed)
    f = np.where(rng.rand(*shape) < fluid_frac, FLUID, EMPTY).astype(np.int32)
    b = bw + 1
    f[:, :, :b] = _SIDE[sides[0]]
    f[:, :, sx - b:] = _SIDE[sides[1]]
    f[:, :b, :] = _SIDE[sides[2]]
    f[:, sy - b:, :] = _SIDE[sides[3]]
    if is3d:
        f[:b] = _SIDE[sides[4]]
        f[sz - b:] = _SIDE[sides[5]]
    k, j, i = _ijk(shape)
    c = rng.uniform(0.35, 0.65, 3) * np.array([sx, sy, sz])
    r = 0.3 * min(sx, sy, sz if is3d else sy)
    d = np.sqrt((i + 0.5 - c[0]) ** 2 + (j + 0.5 - c[1]) ** 2 + ((k + 0.5 - c[2]) ** 2 if is3d else 0.0)) - r
    phi = (d + rng.uniform(-0.4, 0.4, shape)).astype(f32)
    phi[rng.rand(*shape) < zero_frac] = 0
    return f, phi


def rand_mac(dims, seed, scale=1.0):
    sx, sy, sz = dims
    v = np.random.RandomState(seed).uniform(-scale, scale, (3, sz, sy, sx)).astype(f32)
    if sz == 1:
        v[2] = 0
    return v


def loop_inputs(dims):
    """the obstacle loop's start: inflow on x sides, walls elsewhere (boundaryWidth 0), a cylinder (2-D) / sphere (3-D) of
    radius 0.2*sy at (0.25 sx, 0.5 sy, 0.5 sz) joined with the wall levelset; vel = (0.9, 0, 0) plus a seeded y perturbation"""
    sx, sy, sz = dims
    shape = (sz, sy, sx)
    is3d = sz > 1
    f = np.full(shape, EMPTY, np.int32)
    f[:, :, 0] = INFLOW
    f[:, :, sx - 1] = INFLOW
    f[:, 0, :] = OBSTACLE
    f[:, sy - 1, :] = OBSTACLE
    if is3d:
        f[0] = OBSTACLE
        f[sz - 1] = OBSTACLE
    k, j, i = _ijk(shape)
    r = 0.2 * sy
    d = (i + 0.5 - 0.25 * sx) ** 2 + (j + 0.5 - 0.5 * sy) ** 2 + ((k + 0.5 - 0.5 * sz) ** 2 if is3d else 0.0)
    phi = np.sqrt(d) - r
    phi = np.minimum(phi, np.minimum(j - 0.5, sy - 1.5 - j))
    if is3d:
        phi = np.minimum(phi, np.minimum(k - 0.5, sz - 1.5 - k))
    vel = np.zeros((3,) + shape, f32)
    vel[0] = 0.9
    vel[1] = np.random.RandomState(7).uniform(-0.1, 0.1, shape).astype(f32)
    return f, phi.astype(f32), vel


LOOPS = {"loop2d": dict(dims=(128, 64, 1), steps=10), "loop3d": dict(dims=(48, 32, 32), steps=5)}
LOOP_INFLOW = (0.9, 0.0, 0.0)
LOOP_CG = dict(cgAccuracy=1e-4, cgMaxIterFac=5.0)

# the fixture cases of tests/golden/obstacles.npz: name -> (plugin, dims, seed, arguments); see tests/test_obstacles_model.py
CASES = {
    "uf_20x13x11_w0": ("updateFractions", (20, 13, 11), 1, dict(sides="iowwpp", bw=0)),
    "uf_20x13x11_w1": ("updateFractions", (20, 13, 11), 2, dict(sides="pwiopp", bw=1)),
    "uf_24x20x16_w0": ("updateFractions", (24, 20, 16), 3, dict(sides="oiwpip", bw=0)),
    "uf_24x20x16_w1": ("updateFractions", (24, 20, 16), 4, dict(sides="iopwpo", bw=1)),
    "uf_37x29_w0": ("updateFractions", (37, 29, 1), 5, dict(sides="iopw", bw=0)),
    "uf_37x29_w1": ("updateFractions", (37, 29, 1), 6, dict(sides="piow", bw=1)),
    "sof_phi_20x13x11": ("setObstacleFlags", (20, 13, 11), 7, dict(fractions=False, io=False, bw=1)),
    "sof_frac_20x13x11": ("setObstacleFlags", (20, 13, 11), 8, dict(fractions=True, io=False, bw=1)),
    "sof_frac_io_24x20x16": ("setObstacleFlags", (24, 20, 16), 9, dict(fractions=True, io=True, bw=2)),
    "sof_phi_io_37x29": ("setObstacleFlags", (37, 29, 1), 10, dict(fractions=False, io=True, bw=0)),
    "sof_frac_io_37x29": ("setObstacleFlags", (37, 29, 1), 11, dict(fractions=True, io=True, bw=1)),
    "wbf_20x13x11": ("setWallBcs", (20, 13, 11), 12, dict(sides="wwwwww")),
    "wbf_24x20x16": ("setWallBcs", (24, 20, 16), 13, dict(sides="iowwpp")),
    "wbf_37x29": ("setWallBcs", (37, 29, 1), 14, dict(sides="wwww")),
    "infl_xX_20x13x11": ("setInflowBcs", (20, 13, 11), 15, dict(dir="xX", value=(0.9, -0.25, 0.125))),
    "infl_yZ_20x13x11": ("setInflowBcs", (20, 13, 11), 16, dict(dir="yZ", value=(-0.5, 1.5, 2.0))),
    "infl_xX_37x29": ("setInflowBcs", (37, 29, 1), 17, dict(dir="xX", value=(0.9, 0.0, 0.0))),
    "infl_yZ_37x29": ("setInflowBcs", (37, 29, 1), 18, dict(dir="yZ", value=(0.3, -0.7, 0.2))),
    "noise_sdf_20x13x11": ("addNoise", (20, 13, 11), 19, dict(sdf=True, scale=0.1)),
    "noise_20x13x11": ("addNoise", (20, 13, 11), 20, dict(sdf=False, scale=1.0)),
    "noise_sdf_37x29": ("addNoise", (37, 29, 1), 21, dict(sdf=True, scale=0.5)),
}
# NoiseField settings of the addNoise cases (fixedSeed -1, timeAnim 0): posScale, clamp, clampNeg, clampPos
NOISE = dict(posScale=75.0, clamp=True, clampNeg=-1.0, clampPos=1.0)


def case_inputs(name):
    """the seeded inputs of a fixture case: dict of numpy arrays"""
    plugin, dims, seed, a = CASES[name]
    sx, sy, sz = dims
    shape = (sz, sy, sx)
    rng = np.random.RandomState(1000 + seed)
    if plugin == "updateFractions":
        f, phi = scene_inputs(dims, seed, a["sides"], a["bw"])
        return dict(flags=f, phi=phi)
    if plugin == "setObstacleFlags":
        f, phi = scene_inputs(dims, seed, "wiopwp"[:6 if sz > 1 else 4], 0)
        out = dict(flags=f, phi=phi)
        if a["fractions"]:
            fr = np.where(rng.rand(3, *shape) < 0.6, f32(0), rng.uniform(0, 1, (3,) + shape).astype(f32)).astype(f32)
            if sz == 1:
                fr[2] = 0
            out["fractions"] = fr
        if a["io"]:
            out["phiOut"] = rng.uniform(-1, 1, shape).astype(f32)
            out["phiIn"] = rng.uniform(-1, 1, shape).astype(f32)
        return out
    if plugin == "setWallBcs":
        f, phi = scene_inputs(dims, seed, a["sides"], 0, fluid_frac=0.7)
        return dict(flags=f, phi=phi, vel=rand_mac(dims, seed))
    if plugin == "setInflowBcs":
        return dict(vel=rand_mac(dims, seed))
    if plugin == "addNoise":
        f, phi = scene_inputs(dims, seed, "wwwwww", 0)
        out = dict(flags=f, density=rng.uniform(0, 1, shape).astype(f32))
        if a["sdf"]:
            out["sdf"] = phi
        return out
    raise KeyError(name)


def model_case(name, tile=None, params=None):
    """the model's output of a fixture case"""
    plugin, dims, seed, a = CASES[name]
    x = case_inputs(name)
    if plugin == "updateFractions":
        return update_fractions(x["flags"], x["phi"], a["bw"])
    if plugin == "setObstacleFlags":
        return set_obstacle_flags(x["flags"], x["phi"], x.get("fractions"), x.get("phiOut"), x.get("phiIn"), a["bw"])
    if plugin == "setWallBcs":
        return set_wall_bcs_frac(x["flags"], x["vel"], x["phi"])
    if plugin == "setInflowBcs":
        return set_inflow_bcs(x["vel"], a["dir"], a["value"])
    if plugin == "addNoise":
        return add_noise(x["flags"], x["density"], tile, params, x.get("sdf"), a["scale"])
    raise KeyError(name)
