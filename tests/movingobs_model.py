"""numpy statement of moving obstacles and the obstacle coupling (include/open/manta_hip_movingobs.h) and the cases of their tests.

Grids are arrays [z][y][x] (float32 or int32, one component) or [z][y][x][3]; every function rounds where the reference rounds (its
Real is float; a double literal makes an expression double until the next store into a Real).  tools/record_movingobs.py asserts that
these functions reproduce the reference's outputs bit for bit before it writes tests/golden/movingobs.npz; inputs come from the seeded
generators below and are never stored.

ONE PART IS NOT RECORDED.  The reference library the recorder links is the NOPYTHON packaging, in which MovingObstacle::moveLinear
throws "Not yet supported..." at its first applyToGrid (movingobs.cpp:77-83).  For an obstacle that has a shape the recording therefore
holds only what happens before that line: the shapes' new centres (the eased position) and the reset flags.  The stamping of the shapes,
the velocity v and the velocity pass of move_linear() below are written from movingobs.cpp:57-91 and rest on this model alone; the keys
move/<case>/model_* of the golden file are this model's output, stored so that the tests do not depend on the platform's numpy, and are
not a recording.  Calls with alpha outside [0, 1] and obstacles without a shape run to the end in the reference and are recorded whole
(with no shape the velocity pass writes nothing, so they do not cover it either).
"""
import os
import sys
import zlib

import numpy as np

f32, f64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "movingobs.npz")

FLUID, OBSTACLE, EMPTY, INFLOW, OUTFLOW, OPEN, STICK, SURFACE, RESERVED = 1, 2, 4, 8, 16, 32, 64, 128, 256
PDELETE = 1 << 10
DIMS = {"a": (6, 5, 4), "b": (13, 9, 8), "c": (8, 7, 1)}     # (sx, sy, sz); b is more than one workgroup of 256 cells, c is 2-D
EPS2 = f32(1e-6) * f32(1e-6)


def same(a, b):
    """bit for bit, except that a NaN equals any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    u = "u%d" % a.dtype.itemsize
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


def differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return int((a != b).sum())
    u = "u%d" % a.dtype.itemsize
    na, nb = np.isnan(a), np.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(u) != b.view(u)))).sum())


def shape_of(dims, ncomp=1):
    sx, sy, sz = dims
    return (sz, sy, sx) if ncomp == 1 else (sz, sy, sx, ncomp)


def ijk(dims):
    """index arrays K, J, I of shape [z][y][x]"""
    sx, sy, sz = dims
    return np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")


def dims_of(a):
    return a.shape[2], a.shape[1], a.shape[0]


def interior(dims, b=1):
    sx, sy, sz = dims
    K, J, I = ijk(dims)
    m = (I >= b) & (I < sx - b) & (J >= b) & (J < sy - b)
    if sz > 1:
        m &= (K >= b) & (K < sz - b)
    return m


def on_boundary(dims):
    """is_boundary(p, 0), grid.h:447-458"""
    sx, sy, sz = dims
    K, J, I = ijk(dims)
    m = (I <= 0) | (I >= sx - 1) | (J <= 0) | (J >= sy - 1)
    if sz > 1:
        m |= (K <= 0) | (K >= sz - 1)
    return m


# ---- kn_set_wall_bcs2, extforces.cpp:339-368 --------------------------------------------------------------------------------------
def set_wall_bcs2(flags, vel, obvel):
    out = vel.copy()
    fl, ob = (flags & FLUID) != 0, (flags & OBSTACLE) != 0
    is3d = flags.shape[0] > 1
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        if c == 2 and not is3d:
            out[..., 2] = 0
            continue
        cur = tuple(slice(1, None) if a == ax else slice(None) for a in range(3))
        low = tuple(slice(0, -1) if a == ax else slice(None) for a in range(3))
        m = (fl[cur] | fl[low]) & (ob[cur] | ob[low])
        out[cur + (c,)] = np.where(m, obvel[cur + (c,)], out[cur + (c,)])
    return out


# ---- knSetBoundaryMAC / knSetBoundaryMACNorm / kn_set_bound_MAC2, grid.cpp:672-710 ---------------------------------------------------
def set_bound_mac(vel, value, w, rule):
    """rule 0 setBoundMAC, 1 setBoundMAC(normalOnly), 2 set_bound_MAC2"""
    dims = dims_of(vel)
    sx, sy, sz = dims
    K, J, I = ijk(dims)
    z3 = sz > 1
    F = np.zeros(I.shape, bool)
    if rule == 0:
        zin = ((K <= w - 1) | (K >= sz - 1 - w)) if z3 else F
        bx = (I <= w) | (I >= sx - w) | (J <= w - 1) | (J >= sy - 1 - w) | zin
        by = (I <= w - 1) | (I >= sx - 1 - w) | (J <= w) | (J >= sy - w) | zin
        bz = (I <= w - 1) | (I >= sx - 1 - w) | (J <= w - 1) | (J >= sy - 1 - w) | (((K <= w) | (K >= sz - w)) if z3 else F)
    elif rule == 1:
        bx = (I <= w) | (I >= sx - w)
        by = (J <= w) | (J >= sy - w)
        bz = ((K <= w) | (K >= sz - w)) if z3 else F
    else:
        xin, yin = (I <= w) | (I >= sx - 1 - w), (J <= w) | (J >= sy - 1 - w)
        zin = ((K <= w) | (K >= sz - 1 - w)) if z3 else F
        bx = (I <= w + 1) | (I >= sx - 1 - w) | yin | zin
        by = xin | (J <= w + 1) | (J >= sy - 1 - w) | zin
        bz = xin | yin | (((K <= w + 1) | (K >= sz - 1 - w)) if z3 else F)
    out = vel.copy()
    for c, m in enumerate((bx, by, bz)):
        out[..., c] = np.where(m, f32(value[c]), out[..., c])
    return out


# ---- FlagGrid::mark_surface / clear_obstacle, grid.cpp:930-984 -----------------------------------------------------------------------
def mark_surface(flags):
    """the neighbour loop stops at the first neighbour outside the grid, or off the outermost layer and not fluid: the cell is marked
    iff there is one, in any order"""
    dims = dims_of(flags)
    is3d = dims[2] > 1
    fluid = (flags & FLUID) != 0
    stop = ~fluid & ~on_boundary(dims)
    pad = ((1, 1) if is3d else (0, 0), (1, 1), (1, 1))
    P = np.pad(stop, pad, constant_values=True)          # outside the grid: stops the loop
    sz, sy, sx = flags.shape
    mark = np.zeros(flags.shape, bool)
    for dk in ((-1, 0, 1) if is3d else (0,)):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if (di, dj, dk) == (0, 0, 0):
                    continue
                k0 = (1 + dk) if is3d else 0
                mark |= P[k0:k0 + sz, 1 + dj:1 + dj + sy, 1 + di:1 + di + sx]
    out = flags & ~np.int32(SURFACE)
    return np.where(fluid & mark, out | np.int32(SURFACE), out).astype(np.int32)


def clear_obstacle(flags, include_boundary=False):
    m = (flags & OBSTACLE) != 0
    if not include_boundary:
        m &= ~on_boundary(dims_of(flags))
    return np.where(m, np.int32(EMPTY), flags).astype(np.int32)


# ---- knGridClampNorm, grid.cpp:306-312 -------------------------------------------------------------------------------------------
def clamp_norm(a, val):
    val = f32(val)
    a = np.ascontiguousarray(a, f32)
    with np.errstate(all="ignore"):
        if a.ndim == 3:
            n = np.sqrt(a * a)
            return np.where(n > val, a * (val / n), a).astype(f32)
        n = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
        s = val / n
        return np.where((n > val)[..., None], a * s[..., None], a).astype(f32)


# ---- knResetPhiInObs, advection.cpp:397-401 ----------------------------------------------------------------------------------------
def reset_phi_in_obs(flags, sdf):
    return np.where(((flags & OBSTACLE) != 0) & (sdf < 0), f32(0.1), sdf).astype(f32)


# ---- normalize(), vectorbase.h:420-434 ---------------------------------------------------------------------------------------------
def normalize3(n):
    """(the normalised fp32 vector, the norm)"""
    x, y, z = (f32(v) for v in n)
    with np.errstate(all="ignore"):
        l = f32(f32(x * x + y * y) + z * z)
        if abs(float(l) - 1.) < float(EPS2):
            return np.array([x, y, z], f32), f32(1)
        if l > EPS2:
            nrm = f32(np.sqrt(l))
            fac = f32(1. / float(nrm))
            return np.array([x * fac, y * fac, z * fac], f32), nrm
    return np.zeros(3, f32), f32(0)


def dot3(a, b):
    with np.errstate(all="ignore"):
        return f32(f32(f32(a[0]) * f32(b[0]) + f32(a[1]) * f32(b[1])) + f32(a[2]) * f32(b[2]))


# ---- extrapolateMACSimple, fastmarch.cpp:231-375 -----------------------------------------------------------------------------------
def extrapolate_passes(flags, vel, distance, intoObs):
    dims = dims_of(flags)
    dim = 3 if dims[2] > 1 else 2
    inner = interior(dims)
    fl, ob = (flags & FLUID) != 0, (flags & OBSTACLE) != 0
    vel = vel.copy()
    for c in range(dim):
        ax = 2 - c
        mark = fl | np.roll(fl, 1, axis=ax)
        if intoObs:
            mark &= ~ob & ~np.roll(ob, 1, axis=ax)
        tmp = np.where(inner & mark, 1, 0).astype(np.int32)
        comp = vel[..., c].copy()
        for d in range(1, 1 + distance):
            nbs = np.zeros(tmp.shape, np.int32)
            avg = np.zeros(tmp.shape, f32)
            for a, sh in ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))[:2 * dim]:     # +x, -x, +y, -y, +z, -z
                hit = np.roll(tmp, sh, axis=a) == d
                with np.errstate(all="ignore"):
                    avg = np.where(hit, avg + np.roll(comp, sh, axis=a), avg)
                nbs += hit
            upd = inner & (tmp == 0) & (nbs > 0)
            with np.errstate(all="ignore"):
                comp = np.where(upd, avg / np.maximum(nbs, 1).astype(f32), comp)
            tmp = np.where(upd, d + 1, tmp)
        vel[..., c] = comp
    return vel


def get_normal(phi, i, j, k):
    """getNormal, fastmarch.cpp:303-318"""
    sz, sy, sx = phi.shape
    i = 1 if min(i, sx - 2) < 1 else min(i, sx - 2)
    j = 1 if min(j, sy - 2) < 1 else min(j, sy - 2)
    kd = 1
    if sz > 1:
        k = 1 if min(k, sz - 2) < 1 else min(k, sz - 2)
    else:
        kd = 0
    with np.errstate(all="ignore"):
        return np.array([phi[k, j, i + 1] - phi[k, j, i - 1], phi[k, j + 1, i] - phi[k, j - 1, i], phi[k + kd, j, i] - phi[k - kd, j, i]], f32)


def unproject_normal(vel, phi, maxDist, branches=None):
    """knUnprojectNormalComp, fastmarch.cpp:319-332; branches (a dict) counts the cells by what happened to them"""
    dims = dims_of(phi)
    out = vel.copy()
    maxDist = f32(maxDist)
    for k, j, i in zip(*np.nonzero(interior(dims))):
        p = phi[k, j, i]
        if p > 0 or p < -maxDist:
            if branches is not None:
                key = "outside" if p > 0 else "deep"
                branches[key] = branches.get(key, 0) + 1
            continue
        n = get_normal(phi, i, j, k)
        v = vel[k, j, i]
        if dot3(n, v) < 0:
            nn, nrm = normalize3(n)
            l = dot3(nn, v)
            with np.errstate(all="ignore"):
                out[k, j, i] = v - nn * l
            if branches is not None:
                key = "unit" if (nrm == 1 and same(nn, n)) else ("zero" if nrm == 0 else "scaled")
                branches[key] = branches.get(key, 0) + 1
        elif branches is not None:
            branches["away"] = branches.get("away", 0) + 1
    return out


def extrapolate_into_bnd(flags, vel):
    """knExtrapolateIntoBnd, fastmarch.cpp:260-300"""
    sx, sy, sz = dims_of(flags)
    src = vel.copy()
    out = vel.copy()
    for k in range(sz):
        for j in range(sy):
            for i in range(sx):
                if 0 < i < sx - 1 and 0 < j < sy - 1 and (sz == 1 or 0 < k < sz - 1):
                    continue
                c, v = 0, np.zeros(3, f32)
                isObs = (flags[k, j, i] & OBSTACLE) != 0

                def take(kk, jj, ii, comp, neg):
                    w = src[kk, jj, ii].copy()
                    if isObs and ((w[comp] < 0) if neg else (w[comp] > 0)):
                        w[comp] = 0
                    return w
                if i == 0:
                    v, c = take(k, j, i + 1, 0, True), c + 1
                elif i == sx - 1:
                    v, c = take(k, j, i - 1, 0, False), c + 1
                if j == 0:
                    v, c = take(k, j + 1, i, 1, True), c + 1
                elif j == sy - 1:
                    v, c = take(k, j - 1, i, 1, False), c + 1
                if sz > 1:
                    if k == 0:
                        v, c = take(k + 1, j, i, 2, True), c + 1
                    elif k == sz - 1:
                        v, c = take(k - 1, j, i, 2, False), c + 1
                if c > 0:
                    with np.errstate(all="ignore"):
                        out[k, j, i] = v / f32(c)
    return out


def extrapolate_mac_simple(flags, vel, distance=4, phiObs=None, intoObs=False, branches=None):
    v = extrapolate_passes(flags, vel, distance, intoObs)
    if phiObs is not None:
        v = unproject_normal(v, phiObs, distance, branches)
    return extrapolate_into_bnd(flags, v)


# ---- shapes: constructor arguments (8 floats) -> state, setters, isInside ---------------------------------------------------------
class ShapeModel(object):
    """kind 0 Box (args p0, p1), 1 Sphere (centre, radius, scale), 2 Cylinder (centre, radius, z); fp32 members as in shapes.h"""

    def __init__(self, kind, args):
        a = [f32(x) for x in args]
        self.kind = kind
        if kind == 0:
            self.p0, self.p1 = np.array(a[0:3], f32), np.array(a[3:6], f32)
        elif kind == 1:
            self.c, self.r, self.scale = np.array(a[0:3], f32), a[3], np.array(a[4:7], f32)
        else:
            self.c, self.r = np.array(a[0:3], f32), a[3]
            self.setZ(a[4:7])

    def setCenter(self, c):
        c = np.array([f32(x) for x in c], f32)
        if self.kind == 0:
            dh = ((self.p1 - self.p0).astype(f64) * 0.5).astype(f32)
            self.p0, self.p1 = c - dh, c + dh
        else:
            self.c = c

    def setRadius(self, r): self.r = f32(r)

    def setZ(self, z):
        self.zdir, self.zlen = normalize3(z)

    def getCenter(self):
        if self.kind == 0:
            return ((self.p1 + self.p0).astype(f64) * 0.5).astype(f32)
        return self.c

    def state(self):
        """what tools/movingobs_record.cpp reports: 8 floats"""
        o = np.zeros(8, f32)
        if self.kind == 0:
            o[0:3], o[3:6] = self.p0, self.p1
        else:
            o[0:3], o[3] = self.c, self.r
            if self.kind == 2:
                o[4:7] = self.zlen * self.zdir
        return o

    def record(self):
        """the (kind, 12 floats) record of mf_shape_apply_to_grid"""
        q = np.zeros(12, f32)
        if self.kind == 0:
            q[0:3], q[3:6] = self.p0, self.p1
        elif self.kind == 1:
            q[0:3], q[3], q[4:7] = self.c, self.r, self.scale
        else:
            q[0:3], q[3], q[4:7], q[7] = self.c, self.r, self.zdir, self.zlen
        return self.kind, q

    def inside(self, x, y, z):
        """isInside at fp32 positions (arrays), shapes.cpp:151-154, 240-242, 324-329"""
        with np.errstate(all="ignore"):
            if self.kind == 0:
                a, b = self.p0, self.p1
                return (x >= a[0]) & (y >= a[1]) & (z >= a[2]) & (x <= b[0]) & (y <= b[1]) & (z <= b[2])
            if self.kind == 1:
                p, q, r = (x - self.c[0]) / self.scale[0], (y - self.c[1]) / self.scale[1], (z - self.c[2]) / self.scale[2]
                return ((p * p + q * q) + r * r) <= self.r * self.r
            px, py, pz = x - self.c[0], y - self.c[1], z - self.c[2]
            zz = (px * self.zdir[0] + py * self.zdir[1]) + pz * self.zdir[2]
            r2 = ((px * px + py * py) + pz * pz) - zz * zz
            return ~(np.abs(zz) > self.zlen) & (r2 < self.r * self.r)


# ---- MovingObstacle::moveLinear, movingobs.cpp:55-93 ---------------------------------------------------------------------------------
def ease(t, t0, t1, p0, p1, dt, smooth):
    """the host arithmetic of moveLinear in fp32: (alpha, v, pos), or None outside 0 <= alpha <= 1"""
    with np.errstate(all="ignore"):
        t, t0, t1, dt = f32(t), f32(t0), f32(t1), f32(dt)
        alpha = (t - t0) / (t1 - t0)
        if not (alpha >= 0 and alpha <= 1):
            return None
        p0, p1 = np.array([f32(x) for x in p0], f32), np.array([f32(x) for x in p1], f32)
        v = (p1 - p0) / ((t1 - t0) * dt)
        if smooth:
            v = v * (f32(6.0) * (alpha - alpha * alpha))
            alpha = (alpha * alpha) * (f32(3.0) - f32(2.0) * alpha)
        pos = alpha * p1 + (f32(1.0) - alpha) * p0
    return alpha, v.astype(f32), pos.astype(f32)


def move_reset(flags, mid, emptyType):
    """the reset of moveLinear, movingobs.cpp:71-74"""
    return np.where((flags & mid) != 0, np.int32(emptyType), flags).astype(np.int32)


def move_linear(dims, dt, mid, emptyType, shapes, t, t0, t1, p0, p1, smooth, flags, vel):
    """the whole call: (flags, vel) afterwards; the shapes (ShapeModel objects) are moved in place.  The stamping and the velocity pass
    are MODEL ONLY (see the module docstring)."""
    e = ease(t, t0, t1, p0, p1, dt, smooth)
    if e is None:
        return flags.copy(), vel.copy()
    _, v, pos = e
    for sh in shapes:
        sh.setCenter(pos)
    fl = move_reset(flags, mid, emptyType)
    K, J, I = ijk(dims)
    x, y, z = I.astype(f32) + f32(0.5), J.astype(f32) + f32(0.5), K.astype(f32) + f32(0.5)
    for sh in shapes:
        fl = np.where(sh.inside(x, y, z), np.int32(OBSTACLE | mid), fl).astype(np.int32)
    out = vel.copy()
    has = (fl & mid) != 0
    inner = interior(dims)
    is3d = dims[2] > 1
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        low = has if (c == 2 and not is3d) else np.roll(has, 1, axis=ax)     # 2-D: the z stride is 0, flags(i, j, k-1) is the cell
        out[..., c] = np.where(inner & (has | low), v[c], out[..., c])
    return fl, out


# ---- KnProjectParticles, particle.h:552-572 ------------------------------------------------------------------------------------------
class Stream(object):
    """RandomStream (MT19937, init_genrand seeding): getReal() = float(randInt() * (1 / 4294967295))"""

    def __init__(self, seed=3123984):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(int(seed))
        self.drawn = 0

    def real(self):
        self.drawn += 1
        return f32(float(self.bg.random_raw(1)[0]) * (1.0 / 4294967295.0))


def pos_in_grid(dims, p):
    sx, sy, sz = dims
    i, j, k = int(p[0]), int(p[1]), int(p[2])        # truncation toward zero
    r = i >= 0 and j >= 0 and i < sx and j < sy
    return r and ((0 <= k < sz) if sz > 1 else k == 0)


def interpol_vec(grid, p):
    """interpol<Vec3>, interpol.h:52-82, per component"""
    sz, sy, sx = grid.shape[:3]
    with np.errstate(all="ignore"):
        px, py, pz = f32(p[0]) - f32(0.5), f32(p[1]) - f32(0.5), f32(p[2]) - f32(0.5)
        xi, yi, zi = int(px), int(py), int(pz)
        s1 = px - f32(xi); s0 = f32(1. - float(s1))
        t1 = py - f32(yi); t0 = f32(1. - float(t1))
        f1 = pz - f32(zi); f0 = f32(1. - float(f1))
        if px < 0: xi, s0, s1 = 0, f32(1), f32(0)
        if py < 0: yi, t0, t1 = 0, f32(1), f32(0)
        if pz < 0: zi, f0, f1 = 0, f32(1), f32(0)
        if px >= sx - 1: xi, s0, s1 = sx - 2, f32(0), f32(1)
        if py >= sy - 1: yi, t0, t1 = sy - 2, f32(0), f32(1)
        if sz > 1 and pz >= sz - 1: zi, f0, f1 = sz - 2, f32(0), f32(1)
        Z = 1 if sz > 1 else 0                                    # the z stride is 0 in 2-D
        g = lambda dx, dy, dz: grid[zi + dz * Z, yi + dy, xi + dx]
        a = (g(0, 0, 0) * t0 + g(0, 1, 0) * t1) * s0 + (g(1, 0, 0) * t0 + g(1, 1, 0) * t1) * s1
        b = (g(0, 0, 1) * t0 + g(0, 1, 1) * t1) * s0 + (g(1, 0, 1) * t0 + g(1, 1, 1) * t1) * s1
        return (a * f0 + b * f1).astype(f32)


def clampf(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def project_particles(gradient, pos, pflag, stream):
    """the serial loop: positions afterwards.  fp64 where jlen (a double) stands: -dist + jlen * (1 + r) with 1 + r in fp32, each
    component of n * (...) rounded once; jitter = float(jlen * r)"""
    dims = dims_of(gradient)
    out = np.array(pos, f32).reshape(-1, 3).copy()
    for q in range(len(out)):
        if pflag[q] & PDELETE:
            continue
        p = out[q].copy()
        with np.errstate(all="ignore"):
            if pos_in_grid(dims, p):
                n, dist = normalize3(interpol_vec(gradient, p))
                fac = float(-dist) + 0.1 * float(f32(1) + stream.real())
                p = p + (n.astype(f64) * fac).astype(f32)
            jit = np.array([f32(0.1 * float(stream.real())) for _ in range(3)], f32)
            lo, hi = f32(1) + jit, np.array([f32(d - 1) for d in dims], f32) - jit
            out[q] = [clampf(p[c], lo[c], hi[c]) for c in range(3)]
    return out


def gradient_op(phi):
    """GradientOp, commonkernels.h:67-72, on the interior of a zeroed grid"""
    dims = dims_of(phi)
    g = np.zeros(phi.shape + (3,), f32)
    inner = interior(dims)
    with np.errstate(all="ignore"):
        for c, ax in ((0, 2), (1, 1), (2, 0)):
            if c == 2 and dims[2] == 1:
                continue
            d = f32(0.5) * (np.roll(phi, -1, axis=ax) - np.roll(phi, 1, axis=ax))
            g[..., c] = np.where(inner, d, 0)
    return g


def obstacle_levelset(flags):
    """the level set of MovingObstacle::projectOutside, movingobs.cpp:44-47, through tests/reinit_model.py's serial marching"""
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import reinit_model
    dims = dims_of(flags)
    phi = np.where((flags & OBSTACLE) != 0, f32(-0.5), f32(0.5)).astype(f32)
    r = reinit_model.call(dims, phi, flags, None, 6.0, True, False, RESERVED, mode="serial")
    return r["phi"].reshape(flags.shape)


def obstacle_project(flags, pos, pflag, stream):
    return project_particles(gradient_op(obstacle_levelset(flags)), pos, pflag, stream)


# =====================================================================================================================================
# cases: seeded inputs, never stored
# =====================================================================================================================================
def rng(*key):
    """a generator seeded by the key's text"""
    return np.random.RandomState(zlib.crc32("/".join(str(k) for k in key).encode()) & 0x7fffffff)


def rand_flags(name, tag, p_fluid=0.45, p_obs=0.25, extra=0):
    """random fluid / obstacle / empty in EVERY cell, the border included; extra: bits set at random on top"""
    r = rng("flags", name, tag)
    shp = shape_of(DIMS[name])
    u = r.rand(*shp)
    f = np.where(u < p_fluid, FLUID, np.where(u < p_fluid + p_obs, OBSTACLE, EMPTY)).astype(np.int32)
    if extra:
        f |= np.where(r.rand(*shp) < 0.4, extra, 0).astype(np.int32)
    return f


def rand_vec(name, tag, lo=-1.0, hi=1.0):
    r = rng("vec", name, tag)
    return (lo + (hi - lo) * r.rand(*shape_of(DIMS[name], 3))).astype(f32)


def rand_real(name, tag, lo=-1.0, hi=1.0):
    r = rng("real", name, tag)
    return (lo + (hi - lo) * r.rand(*shape_of(DIMS[name]))).astype(f32)


def domain_flags(name):
    """walls on the outermost layer, empty inside"""
    f = np.full(shape_of(DIMS[name]), EMPTY, np.int32)
    f[on_boundary(DIMS[name])] = OBSTACLE
    return f


# set_wall_bcs2
def wall2_inputs(name):
    return rand_flags(name, "wall2"), rand_vec(name, "wall2v"), rand_vec(name, "wall2o", 2.0, 3.0)


# setBoundMAC / set_bound_MAC2: width 3 makes opposite bands overlap (2w + 3 > size) along at least one axis of every grid
BOUND_WIDTHS = (0, 1, 2, 3)
BOUND_VALUE = (f32(7.5), f32(-8.25), f32(9.125))


def bound_input(name):
    return rand_vec(name, "bound")


# mark_surface
SURF_KINDS = ("rand", "diag")


def surf_input(name, kind):
    dims = DIMS[name]
    if kind == "rand":
        # mostly fluid, the border cells included; obstacles and empties among them; stale TypeSurface on cells of every type
        return rand_flags(name, "surf", p_fluid=0.8, p_obs=0.1, extra=SURFACE)
    # all fluid but one empty cell off the border: its diagonal neighbours have no other non-fluid neighbour
    f = np.full(shape_of(dims), FLUID, np.int32)
    f[(dims[2] // 2), dims[1] // 2, dims[0] // 2] = EMPTY | SURFACE
    return f


# clear_obstacle
def clear_input(name):
    return rand_flags(name, "clear", extra=STICK)


# clamp_norm
CNORM_VALS = (0.0, 0.5, 1.25, 100.0)


def cnorm_input(name, kind):
    """norms below, at (0.5 exactly) and above the values; zeros"""
    if kind == "real":
        a = rand_real(name, "cnorm", -2.0, 2.0)
        flat = a.reshape(-1)
        flat[0], flat[1], flat[2], flat[3] = 0.0, 0.5, -0.5, -0.0
    else:
        a = rand_vec(name, "cnorm", -1.5, 1.5)
        flat = a.reshape(-1, 3)
        flat[0] = 0
        flat[1] = (0.5, 0, 0)
        flat[2] = (0, 0, -0.5)
        flat[3] = (0.3, 0.4, 0)
    return a


# resetPhiInObs
def reset_inputs(name):
    return rand_flags(name, "reset"), rand_real(name, "resetphi")


# extrapolateMACSimple(phiObs)
EXTRAP_DISTANCE = 2


def extrap_inputs(name):
    """(flags, vel, phiObs, planted cells).  flags: walls, a slab of fluid at i = 1, an obstacle box beside it; phiObs in [-4, 2] (> 0,
    < -distance and between).  On the grids that are wide enough two cells out of the passes' reach are planted: one whose normal is
    exactly (1, 0, 0) and one whose normal is tiny (normalize gives zero), both with a velocity against it."""
    dims = DIMS[name]
    sx, sy, sz = dims
    K, J, I = ijk(dims)
    f = domain_flags(name)
    f[(f == EMPTY) & (I < 2)] = FLUID
    box = (I >= 2) & (I <= 3) & (J >= 2) & (J <= 3) & ((K >= 1) | (sz == 1))
    f[box & ~on_boundary(dims)] = OBSTACLE
    vel = rand_vec(name, "extrapv")
    phi = rand_real(name, "extrapphi", -4.0, 2.0)
    k = sz // 2 if sz > 1 else 0
    planted = []
    if sx >= 8:
        ci = sx - 3
        for cj, centre, hi_, lo_ in ((sy - 3, -0.5, 0.25, -0.75), (1, 0.0, 1e-7, 0.0)):
            phi[k, cj, ci] = centre
            phi[k, cj, ci + 1], phi[k, cj, ci - 1] = hi_, lo_
            phi[k, cj + 1, ci] = phi[k, cj - 1, ci] = lo_
            if sz > 1:
                phi[k + 1, cj, ci] = phi[k - 1, cj, ci] = lo_
            vel[k, cj, ci] = (-1.0, 0.3, 0.2)
            planted.append((k, cj, ci))
    return f, vel, phi, planted


# shapes' setters
SETTER_CASES = [
    (0, (1.1, 2.3, 0.7, 4.9, 3.1, 2.9, 0, 0), (5.3, 4.7, 3.9), 0, 0.0, (0, 0, 0)),
    (0, (0.1, 0.2, 0.3, 0.7, 0.9, 1.3, 0, 0), (1.0 / 3.0, 2.0 / 3.0, 0.1), 0, 0.0, (0, 0, 0)),
    (1, (3.3, 2.2, 1.1, 1.7, 1, 1, 1, 0), (0.1, 0.7, 1.0 / 3.0), 0, 0.0, (0, 0, 0)),
    (2, (3.3, 2.2, 1.1, 1.7, 0.3, 1.9, 0.2, 0), (0.1, 0.7, 1.0 / 3.0), 0, 0.0, (0, 0, 0)),
    (2, (3.3, 2.2, 1.1, 1.7, 0, 1, 0, 0), (4.1, 0.7, 2.0), 1, 0.3, (1.3, 0.1, 2.7)),
    (2, (3.3, 2.2, 1.1, 1.7, 0, 2, 0, 0), (4.1, 0.7, 2.0), 1, 2.3, (0, 0, 1)),
    (2, (3.3, 2.2, 1.1, 1.7, 0, 2, 0, 0), (4.1, 0.7, 2.0), 1, 2.3, (0, 0, 0)),
]


def setters_model(kind, args, centre, doCyl, r, z):
    sh = ShapeModel(kind, args)
    sh.setCenter(centre)
    if kind == 2 and doCyl:
        sh.setRadius(r)
        sh.setZ(z)
    return sh.state(), sh.getCenter().astype(f32)


# moveLinear
MOVE_DT = 0.4
MOVE_EMPTY = EMPTY | STICK        # an emptyType other than FlagEmpty, for the cases that say so


def move_cases():
    """name -> dict(grid, which (ID index), emptyType, shapes [(kind, args)], t, t0, t1, p0, p1, smooth)"""
    box_b = (0, (3.0, 2.0, 2.0, 6.2, 5.0, 5.1, 0, 0))
    sph_b = (1, (6.0, 4.0, 4.0, 2.3, 1, 1.5, 1, 0))
    cyl_b = (2, (6.0, 4.0, 4.0, 1.6, 0.5, 2.0, 0.3, 0))
    box_c = (0, (2.0, 2.0, 0.0, 4.5, 4.2, 1.0, 0, 0))
    sph_c = (1, (4.0, 3.0, 0.5, 1.8, 1, 1, 1, 0))
    box_a = (0, (1.0, 1.0, 1.0, 3.5, 2.6, 2.6, 0, 0))
    pb0, pb1 = (4.2, 3.6, 3.1), (8.4, 5.2, 4.9)
    pc0, pc1 = (2.6, 2.4, 0.5), (5.3, 4.4, 0.5)
    C = {}
    for tag, t in (("below", 0.9), ("at0", 1.0), ("inside", 1.7), ("at1", 3.0), ("above", 3.1)):
        for smooth in (0, 1):
            C["b/%s/s%d" % (tag, smooth)] = dict(grid="b", which=1, emptyType=EMPTY, shapes=[box_b, sph_b], t=t, t0=1.0, t1=3.0, p0=pb0, p1=pb1, smooth=smooth)
    C["b/cyl"] = dict(grid="b", which=0, emptyType=MOVE_EMPTY, shapes=[cyl_b, box_b], t=2.2, t0=1.0, t1=3.0, p0=pb0, p1=pb1, smooth=1)
    C["b/noshape"] = dict(grid="b", which=2, emptyType=MOVE_EMPTY, shapes=[], t=2.2, t0=1.0, t1=3.0, p0=pb0, p1=pb1, smooth=1)
    C["a/box"] = dict(grid="a", which=4, emptyType=EMPTY, shapes=[box_a], t=0.5, t0=0.0, t1=1.0, p0=(2.2, 1.9, 1.8), p1=(3.4, 2.7, 2.2), smooth=0)
    C["c/inside"] = dict(grid="c", which=3, emptyType=MOVE_EMPTY, shapes=[box_c, sph_c], t=0.25, t0=0.0, t1=1.0, p0=pc0, p1=pc1, smooth=1)
    C["c/above"] = dict(grid="c", which=3, emptyType=EMPTY, shapes=[box_c], t=1.25, t0=0.0, t1=1.0, p0=pc0, p1=pc1, smooth=1)
    C["c/noshape"] = dict(grid="c", which=0, emptyType=EMPTY, shapes=[], t=0.5, t0=0.0, t1=1.0, p0=pc0, p1=pc1, smooth=0)
    return C


def move_id(which):
    return 1 << (10 + which)


def move_inputs(case):
    """flags: walls, fluid, and cells that carry this obstacle's ID (to be reset) and ANOTHER obstacle's ID (to survive); vel random"""
    c = move_cases()[case]
    name = c["grid"]
    r = rng("move", case)
    f = domain_flags(name)
    shp = f.shape
    u = r.rand(*shp)
    inner = interior(DIMS[name])
    f[inner & (u < 0.5)] = FLUID
    mine, other = move_id(c["which"]), move_id((c["which"] + 1) % 5)
    f[inner & (u >= 0.5) & (u < 0.65)] = OBSTACLE | mine
    f[inner & (u >= 0.65) & (u < 0.8)] = OBSTACLE | other
    f[0, 0, 0] |= mine                                   # a border cell that carries the ID is reset as well
    return f, rand_vec(name, "move" + case)


def move_model(case):
    """(flags, vel, states [nshapes][8]) after the call"""
    c = move_cases()[case]
    f, v = move_inputs(case)
    shapes = [ShapeModel(k, a) for k, a in c["shapes"]]
    fl, vel = move_linear(DIMS[c["grid"]], MOVE_DT, move_id(c["which"]), c["emptyType"], shapes, c["t"], c["t0"], c["t1"], c["p0"], c["p1"],
                          bool(c["smooth"]), f, v)
    return fl, vel, np.array([s.state() for s in shapes], f32).reshape(len(shapes), 8)


# projectOutside: ONE sequence, in this order, on one stream that is never reseeded
def particles(name, n, tag):
    """n positions in and around the grid, about one in seven deleted; in 2-D z = 0.5 except for a few off-plane ones"""
    sx, sy, sz = DIMS[name]
    r = rng("parts", name, n, tag)
    pos = np.stack([r.uniform(-1.0, d + 1.0, n) for d in (sx, sy, sz)], axis=1).astype(f32)
    if sz == 1:
        pos[:, 2] = np.where(r.rand(n) < 0.85, 0.5, pos[:, 2])
    flag = np.where(r.rand(n) < 0.15, PDELETE, 0).astype(np.int32) | np.where(r.rand(n) < 0.3, 1, 0).astype(np.int32)
    return pos.reshape(n, 3), flag


def gradient_input(name):
    """a random Vec3 grid with zero vectors, a unit vector and a tiny vector in it"""
    g = rand_vec(name, "grad", -1.2, 1.2)
    flat = g.reshape(-1, 3)
    r = rng("gradz", name)
    flat[r.rand(len(flat)) < 0.2] = 0
    flat[5] = (0, 1, 0)
    flat[6] = (1e-7, 0, 0)
    return g


def obstacle_flags(name):
    dims = DIMS[name]
    sx, sy, sz = dims
    K, J, I = ijk(dims)
    f = domain_flags(name)
    body = (I >= sx // 2 - 1) & (I <= sx // 2 + 1) & (J >= 2) & (J <= sy - 4) & ((sz == 1) | ((K >= 2) & (K <= sz - 3)))
    f[body] = OBSTACLE | move_id(0)
    f[(f == EMPTY) & (J < sy // 2)] = FLUID
    return f


PROJECT_SEQUENCE = [("grad", "b", 0), ("grad", "b", 1), ("grad", "b", 65), ("grad", "b", 300), ("grad", "b", 300), ("grad", "c", 65), ("grad", "a", 65),
                    ("obs", "b", 300), ("obs", "c", 65)]
"""(what, grid, particles): BasicParticleSystem.projectOutside on a random gradient, or MovingObstacle.projectOutside.  The two
300-particle calls in a row have the same input and different draws."""


def project_step(q, stream):
    """the output of step q of the sequence, drawn from `stream` (which must have served steps 0 .. q-1)"""
    what, name, n = PROJECT_SEQUENCE[q]
    pos, flag = particles(name, n, what)
    if what == "grad":
        return project_particles(gradient_input(name), pos, flag, stream)
    return obstacle_project(obstacle_flags(name), pos, flag, stream)


# ---- the end-to-end loop: MODEL PARITY (moveLinear's stamping and velocity are model-only) -------------------------------------------
LOOP = dict(grid="b", steps=10, dt=0.5, t0=0.0, t1=5.0, p0=(3.6, 3.2, 3.1), p1=(8.9, 5.4, 4.6), box=(0, (2.0, 2.0, 2.0, 4.6, 4.4, 4.2, 0, 0)), which=0,
            particles=120, distance=2)
"""per step: moveLinear(t = step * dt), set_wall_bcs2 with obvel = the moved velocity field, setBoundMAC(0, 0), mark_surface,
extrapolateMACSimple(distance, phiObs = the box's rough level set, intoObs), resetPhiInObs, clamp_norm(vel, 1.5),
MovingObstacle.projectOutside.  The loop has no pressure solve: it strings the new entries together, nothing else."""


def loop_inputs():
    name = LOOP["grid"]
    f = domain_flags(name)
    K, J, I = ijk(DIMS[name])
    f[(f == EMPTY) & (J < DIMS[name][1] // 2 + 1)] = FLUID
    vel = rand_vec(name, "loopv", -2.0, 2.0)
    phi = rand_real(name, "loopphi", -1.0, 1.0)
    pos, flag = particles(name, LOOP["particles"], "loop")
    return f, vel, phi, pos, flag


def loop_model():
    """the end state: dict(flags, vel, obvel, phi, pos)"""
    name = LOOP["grid"]
    dims = DIMS[name]
    flags, vel, phi, pos, pflag = loop_inputs()
    stream = Stream()
    box = ShapeModel(*LOOP["box"])
    mid = move_id(LOOP["which"])
    obvel = np.zeros_like(vel)
    for step in range(LOOP["steps"]):
        t = f32(step) * f32(LOOP["dt"])
        flags, obvel = move_linear(dims, LOOP["dt"], mid, EMPTY, [box], t, LOOP["t0"], LOOP["t1"], LOOP["p0"], LOOP["p1"], True, flags, obvel)
        vel = set_wall_bcs2(flags, vel, obvel)
        vel = set_bound_mac(vel, (f32(0), f32(0), f32(0)), 0, 0)
        flags = mark_surface(flags)
        phiObs = np.where((flags & mid) != 0, f32(-1.0), f32(1.0)).astype(f32)
        vel = extrapolate_mac_simple(flags, vel, LOOP["distance"], phiObs, True)
        phi = reset_phi_in_obs(flags, phi)
        vel = clamp_norm(vel, 1.5)
        pos = obstacle_project(flags, pos, pflag, stream)
    return dict(flags=flags, vel=vel, obvel=obvel, phi=phi, pos=pos)
