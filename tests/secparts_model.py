"""numpy model of the secondary particles (source/plugin/secondaryparticles.cpp): the potentials (:24-103), the sampling of new
particles (:105-220) both as the literal serial loop over the cells with one running random stream and as the order-free
statement the HIP kernels implement, the per-type update in "linear" and "cubic" mode (:225-447), flipDeleteParticlesInObstacle
(:450-476), setFlagsFromLevelset / setMACFromLevelset (:512-533) -- plus the seeded input generators of the fixture cases of
tests/golden/secparts.npz (inputs are regenerated, never stored).

Layout: scalar grids [z][y][x], Vec3 / MAC grids [z][y][x][3], particle positions [n][3]; everything fp32 / int32, every operation
rounded where the reference rounds (fp64 where an operand is a double literal, util/vectorbase.h for norm / getNormalized).
cos / sin of the azimuth are numpy's fp64 functions rounded once to fp32: the reference's are glibc's cosf / sinf, so sampled
positions and velocities are compared within `sample_bound`, everything else bit for bit.
"""
import numpy as np

import nbflip_model as N
from nbflip_model import Channel, Parts, interp_mac, interp_real

f32, f64 = np.float32, np.float64
PSPRAY, PBUBBLE, PFOAM, PTRACER, PDELETE = 2, 4, 8, 16, 1 << 10
TypeFluid, TypeObstacle, TypeEmpty, TypeInflow, TypeOutflow = 1, 2, 4, 8, 16
JTYPE = TypeObstacle | TypeOutflow | TypeInflow
EPS2 = f32(1e-6) * f32(1e-6)
INT_MIN = -(1 << 31)


# ---------------------------------------------------------------------------------------------------------------------------------
# util/vectorbase.h
# ---------------------------------------------------------------------------------------------------------------------------------
def _l2(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]).astype(f32)


def normalized(v):
    """getNormalized, :404-416: in the header's template sqrt(l) is the double function, so fac = Real(1. / sqrt(double(l)))"""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        l = _l2(v)
        near1 = np.abs(l.astype(f64) - 1.) < f64(EPS2)
        fac = (1. / np.sqrt(l.astype(f64))).astype(f32)
        scaled = (v * fac[..., None]).astype(f32)
    return np.where(near1[..., None], v, np.where((l > EPS2)[..., None], scaled, f32(0))).astype(f32)


def norm(v):
    """norm, :384-389"""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        l = _l2(v)
        near1 = np.abs(l.astype(f64) - 1.) < f64(EPS2)
        return np.where(l <= EPS2, f32(0), np.where(near1, f32(1), np.sqrt(l))).astype(f32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]).astype(f32)


def to_int(p):
    """(int)Real as x86-64 converts it: truncation; NaN and out of range give INT_MIN"""
    p = np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        ok = (p >= f32(-2147483648.)) & (p < f32(2147483648.))
        return np.where(ok, np.where(ok, p, 0).astype(np.int64), INT_MIN)


def in_bounds(c, dims, bnd):
    """GridBase::isInBounds(Vec3i, bnd): a 2-D grid has the plane z == 0 only"""
    sx, sy, sz = dims
    r = (c[..., 0] >= bnd) & (c[..., 1] >= bnd) & (c[..., 0] < sx - bnd) & (c[..., 1] < sy - bnd)
    if sz > 1:
        return r & (c[..., 2] >= bnd) & (c[..., 2] < sz - bnd)
    return r & (c[..., 2] == 0)


def _dims(g):
    return (g.shape[2], g.shape[1], g.shape[0])


def _cells(dims):
    sx, sy, sz = dims
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    return i, j, k


# ---------------------------------------------------------------------------------------------------------------------------------
# potentials
# ---------------------------------------------------------------------------------------------------------------------------------
def clamp_potential(p, tmin, tmax):
    """:25-27 with std::min(a, b) = b < a ? b : a"""
    with np.errstate(all="ignore"):
        a = np.where(tmax < p, tmax, p)
        b = np.where(tmin < p, tmin, p)
        return ((a - b).astype(f32) / (tmax - tmin)).astype(f32)


def centered(vel):
    """MACGrid::getCentered on the cells that have their upper faces in the grid; NaN elsewhere"""
    sz, sy, sx = vel.shape[:3]
    c = np.full(vel.shape, np.nan, f32)
    c[:, :, :-1, 0] = f32(0.5) * (vel[:, :, :-1, 0] + vel[:, :, 1:, 0])
    c[:, :-1, :, 1] = f32(0.5) * (vel[:, :-1, :, 1] + vel[:, 1:, :, 1])
    if sz > 1:
        c[:-1, :, :, 2] = f32(0.5) * (vel[:-1, :, :, 2] + vel[1:, :, :, 2])
        c[-1, :, :, 2] = np.nan
    else:
        c[..., 2] = 0
    return c


def gradient(normal, phi):
    """GradientOp, commonkernels.h:67-72: the interior; the border keeps the caller's values"""
    out = np.array(normal, f32)
    sz = phi.shape[0]
    zs = slice(1, -1) if sz > 1 else slice(None)
    out[zs, 1:-1, 1:-1, 0] = f32(0.5) * (phi[zs, 1:-1, 2:] - phi[zs, 1:-1, :-2])
    out[zs, 1:-1, 1:-1, 1] = f32(0.5) * (phi[zs, 2:, 1:-1] - phi[zs, :-2, 1:-1])
    out[zs, 1:-1, 1:-1, 2] = f32(0.5) * (phi[2:, 1:-1, 1:-1] - phi[:-2, 1:-1, 1:-1]) if sz > 1 else f32(0)
    return out


def potentials(flags, vel, normal, phi, radius, tauMinTA, tauMaxTA, tauMinWC, tauMaxWC, tauMinKE, tauMaxKE, scaleFromManta,
               itype=TypeFluid, jtype=JTYPE, raw=None):
    """flipComputeSecondaryParticlePotentials: returns potTA, potWC, potKE, neighborRatio, normal.  Vectorised over the cells; the
    neighbours are visited x outer, y, z inner, which is the order of the fp32 sums."""
    assert radius >= 1
    flags = np.asarray(flags, np.int32)
    dims = sx, sy, sz = _dims(flags)
    is3d = sz > 1
    r = int(radius)
    scale = f32(scaleFromManta)
    taus = [f32(t) for t in (tauMinTA, tauMaxTA, tauMinWC, tauMaxWC, tauMinKE, tauMaxKE)]
    normal = gradient(normal, np.asarray(phi, f32))
    out = [np.zeros(flags.shape, f32) for _ in range(4)]
    if sx <= 2 * r or sy <= 2 * r or (is3d and sz <= 2 * r):
        return out[0], out[1], out[2], out[3], normal
    with np.errstate(all="ignore"):
        sv = (scale * centered(np.asarray(vel, f32))).astype(f32)
        sn = normalized(normal)
        i, j, k = _cells(dims)
        xs = np.stack([scale * i.astype(f32), scale * j.astype(f32), scale * k.astype(f32)], axis=-1).astype(f32)
        inb = in_bounds(np.stack([i, j, k], axis=-1), dims, 1)
        h = f32((1.732 if is3d else 1.414) * r)
        rz = r if is3d else 0

        def reg(a, dx=0, dy=0, dz=0):
            return a[rz + dz:sz - rz + dz, r + dy:sy - r + dy, r + dx:sx - r + dx]

        xi, vi, ni = reg(xs), reg(sv), reg(sn)
        vdiff, kappa = np.zeros(xi.shape[:3], f32), np.zeros(xi.shape[:3], f32)
        cf, cm = np.zeros(xi.shape[:3], np.int64), np.zeros(xi.shape[:3], np.int64)
        for dx in range(-r, r + 1):
            for dy in range(-r, r + 1):
                for dz in range(-rz, rz + 1):
                    if dx == 0 and dy == 0 and dz == 0:
                        continue
                    fj = reg(flags, dx, dy, dz)
                    ok = reg(inb, dx, dy, dz) & ((fj & jtype) == 0)
                    cf += ok & ((fj & itype) != 0)
                    cm += ok
                    xij = (xi - reg(xs, dx, dy, dz)).astype(f32)
                    vij = (vi - reg(sv, dx, dy, dz)).astype(f32)
                    nj = reg(sn, dx, dy, dz)
                    uxij = normalized(xij)
                    fall = (f32(1) - norm(xij) / h).astype(f32)
                    t = (norm(vij) * (f32(1) - dot(normalized(vij), uxij)) * fall).astype(f32)
                    vdiff = np.where(ok, (vdiff + t).astype(f32), vdiff)
                    t = ((f32(1) - dot(ni, nj)) * fall).astype(f32)
                    kappa = np.where(ok & (dot(uxij, ni) < 0), (kappa + t).astype(f32), kappa)
        me = (reg(flags) & itype) != 0
        ratio = cf.astype(f32) / cm.astype(f32)
        ta = clamp_potential(vdiff, taus[0], taus[1])
        wc = np.where(dot(normalized(vi), ni).astype(f64) >= 0.6, clamp_potential(kappa, taus[2], taus[3]), f32(0))
        ke = clamp_potential((f32(62.5) * _l2(vi)).astype(f32), taus[4], taus[5])
        if raw is not None:
            raw.update(cells=me, vdiff=vdiff, kappa=kappa, ek=(f32(62.5) * _l2(vi)).astype(f32), count=cm,
                       gate=dot(normalized(vi), ni).astype(f64) >= 0.6, vi=vi, ni=ni)
        for o, v in zip(out, (ta, wc, ke, ratio)):
            reg(o)[...] = np.where(me, v, f32(0))
    return out[0], out[1], out[2], out[3], normal


# ---------------------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------------------
class Stream(object):
    """RandomStream(9832) with a cursor: the `static RandomStream mRand` of one sampling kernel"""

    def __init__(self, cursor=0):
        self.bg = np.random.MT19937()
        self.bg._legacy_seeding(9832)
        self.cursor = 0
        self.take(cursor)

    def take(self, n):
        self.cursor += n
        return (self.bg.random_raw(n).astype(f64) * (1.0 / 4294967295.0)).astype(f32)


def sample_entries(mode, flags, potTA, potWC, potKE, k_ta, k_wc, dt, itype=TypeFluid):
    """per entry (a cell, or one of its 8 cylinders in x, y, z loop order): cell index, cylinder centre / cell corner, the
    potentials there and n = int(KE * (k_ta * TA + k_wc * WC) * dt); 0 where the cell is no itype cell"""
    flags = np.asarray(flags, np.int32)
    dims = _dims(flags)
    i, j, k = (a.ravel() for a in _cells(dims))
    cell = np.arange(i.size)
    if mode == "single":
        xi = np.stack([i, j, k], axis=1).astype(f32)
        KE, TA, WC = (np.asarray(p, f32).ravel() for p in (potKE, potTA, potWC))
    else:
        cell = np.repeat(cell, 8)
        sub = np.tile(np.arange(8), i.size)
        base = (np.stack([i, j, k], axis=1).astype(f32) - f32(0.25)).astype(f32)
        hi = np.stack([(sub >> 2) & 1, (sub >> 1) & 1, sub & 1], axis=1).astype(bool)
        xi = np.repeat(base, 8, axis=0)
        xi = np.where(hi, (xi + f32(0.5)).astype(f32), xi)
        KE, TA, WC = (interp_real(np.asarray(p, f32), xi) for p in (potKE, potTA, potWC))
    with np.errstate(all="ignore"):
        val = ((KE * (f32(k_ta) * TA + f32(k_wc) * WC).astype(f32)).astype(f32) * f32(dt)).astype(f32)
    n = np.where((flags.ravel()[cell] & itype) != 0, to_int(val), 0)
    return dict(cell=cell, xi=xi, KE=KE, TA=TA, WC=WC, n=n)


def _emit(mode, is3d, vel, xi, KE, TA, WC, R, ratio_cell, lMin, lMax, c_s, c_b, dt):
    """the body of the `for di` loop for a batch of particles: R [m][4] are the particle's reals (r, theta, h, lifetime)"""
    dt = f32(dt)
    with np.errstate(all="ignore"):
        vi = interp_mac(vel, xi)
        dirv = (dt * vi).astype(f32)
        zero = np.zeros(len(xi), f32)
        e1 = normalized(np.stack([dirv[:, 2], zero, -dirv[:, 0]], axis=1))
        cr = np.stack([e1[:, 1] * dirv[:, 2] - e1[:, 2] * dirv[:, 1], e1[:, 2] * dirv[:, 0] - e1[:, 0] * dirv[:, 2],
                       e1[:, 0] * dirv[:, 1] - e1[:, 1] * dirv[:, 0]], axis=1).astype(f32)
        e2 = normalized(cr)
        r = (f32(0.5 if mode == "single" else 0.25) * np.sqrt(R[:, 0])).astype(f32)
        theta = ((R[:, 1] * f32(2)).astype(f32).astype(f64) * np.pi).astype(f32)
        h = (R[:, 2] * norm(dirv)).astype(f32)
        ct, st = np.cos(theta.astype(f64)).astype(f32), np.sin(theta.astype(f64)).astype(f32)
        A = ((r * ct).astype(f32)[:, None] * e1).astype(f32)
        B = ((r * st).astype(f32)[:, None] * e2).astype(f32)
        xd = (((xi + A).astype(f32) + B).astype(f32) + (h[:, None] * normalized(vi)).astype(f32)).astype(f32)
        if not is3d:
            xd[:, 2] = 0
        v = ((A + B).astype(f32) + vi).astype(f32)
        temp = (((KE + TA).astype(f32) + WC).astype(f32) / f32(3)).astype(f32)
        l = ((((f32(lMax) - f32(lMin)) * temp).astype(f32) + f32(lMin)).astype(f32).astype(f64) + R[:, 3].astype(f64) * 0.1).astype(f32)
        flag = np.where(ratio_cell < f32(c_s), PSPRAY, np.where(ratio_cell > f32(c_b), PBUBBLE, PFOAM)).astype(np.int32)
    return dict(pos=xd, vel=v, life=l, flag=flag, r=r)


def sample_orderfree(mode, flags, vel, potTA, potWC, potKE, ratio, lMin, lMax, c_s, c_b, k_ta, k_wc, dt, stream, itype=TypeFluid):
    """counts, exclusive scans for the particle and the stream offsets, the stream window, then every particle on its own"""
    E = sample_entries(mode, flags, potTA, potWC, potKE, k_ta, k_wc, dt, itype)
    single = mode == "single"
    n = E["n"]
    npos = np.maximum(n, 0)
    rcount = 4 * npos + (3 * (n != 0) if single else 0)
    poff = np.cumsum(npos) - npos
    roff = np.cumsum(rcount) - rcount
    reals = stream.take(int(rcount.sum()))
    e = np.repeat(np.arange(n.size), npos)
    di = np.arange(e.size) - poff[e]
    xi = E["xi"][e]
    rb = roff[e]
    if single:
        xi = (xi + np.stack([reals[rb], reals[rb + 1], reals[rb + 2]], axis=1)).astype(f32)
        rb = rb + 3
    rb = rb + 4 * di
    R = np.stack([reals[rb + q] for q in range(4)], axis=1) if e.size else np.zeros((0, 4), f32)
    out = _emit(mode, flags.shape[0] > 1, np.asarray(vel, f32), xi, E["KE"][e], E["TA"][e], E["WC"][e], R,
                np.asarray(ratio, f32).ravel()[E["cell"][e]], lMin, lMax, c_s, c_b, dt)
    out["reals"] = int(rcount.sum())
    return out


def sample_serial(mode, flags, vel, potTA, potWC, potKE, ratio, lMin, lMax, c_s, c_b, k_ta, k_wc, dt, stream, itype=TypeFluid):
    """the reference's loop: the entries in order, every real drawn from the running stream where the loop draws it"""
    E = sample_entries(mode, flags, potTA, potWC, potKE, k_ta, k_wc, dt, itype)
    single = mode == "single"
    is3d = flags.shape[0] > 1
    vel = np.asarray(vel, f32)
    rat = np.asarray(ratio, f32).ravel()
    parts, start = [], stream.cursor
    for e in np.nonzero(E["n"])[0]:
        n = int(E["n"][e])
        xi = E["xi"][e:e + 1]
        if single:
            xi = (xi + stream.take(3)[None, :]).astype(f32)
        for di in range(n):
            R = stream.take(4)[None, :]
            parts.append(_emit(mode, is3d, vel, xi, E["KE"][e:e + 1], E["TA"][e:e + 1], E["WC"][e:e + 1], R, rat[E["cell"][e:e + 1]],
                               lMin, lMax, c_s, c_b, dt))
    keys = ("pos", "vel", "life", "flag", "r")
    if parts:
        out = {q: np.concatenate([p[q] for p in parts]) for q in keys}
    else:
        out = dict(pos=np.zeros((0, 3), f32), vel=np.zeros((0, 3), f32), life=np.zeros(0, f32), flag=np.zeros(0, np.int32), r=np.zeros(0, f32))
    out["reals"] = stream.cursor - start
    return out


def sample(parts, iv, il, new):
    """append the sampled particles: add() -> addEntry() gives every channel a zero entry; v_sec (channel iv) and l_sec (il) are set"""
    m = len(new["flag"])
    if not m:
        return
    parts.pos = np.concatenate([parts.pos, new["pos"]])
    parts.flag = np.concatenate([parts.flag, new["flag"]])
    for q, c in enumerate(parts.channels):
        add = new["vel"] if q == iv else (new["life"] if q == il else np.zeros((m,) + c.data.shape[1:], c.data.dtype))
        c.data = np.concatenate([c.data, add.astype(c.data.dtype)])
    parts.chunk = parts.size() // N.DELETE_PART


def ulp(x):
    """2^(floor(log2 |x|) - 23); the spacing of the smallest normal for 0 and subnormals"""
    a = np.maximum(np.abs(np.asarray(x, f64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def sample_bound(r, ref):
    """4 r 2^-23 + 3 ulp(reference value), per component; r [m], ref [m][3]"""
    return 4.0 * np.asarray(r, f64)[:, None] * 2.0 ** -23 + 3.0 * ulp(ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------------------
def cubic_spline(h, l, dim):
    """:226-233: h2, h3, q, square(q), cubed(q) are Real; the constants and the polynomial are double, narrowed on return"""
    h = f32(h)
    h2 = f32(h * h)
    h3 = f32(h2 * h)
    c = f32(1e0 / (np.pi * f64(h3))) if dim == 3 else f32(10e0 / (7e0 * np.pi * f64(h2)))
    with np.errstate(all="ignore"):
        q = (l / h).astype(f32)
        sq, cu = (q * q).astype(f32), ((q * q).astype(f32) * q).astype(f32)
        w1 = (f64(c) * (1e0 - 1.5 * sq.astype(f64) + 0.75 * cu.astype(f64))).astype(f32)
        t = 2e0 - q.astype(f64)
        w2 = (f64(c) * (0.25 * (t * t * t))).astype(f32)
        q64 = q.astype(f64)
        return np.where(q64 < 1e0, w1, np.where(q64 < 2e0, w2, f32(0))).astype(f32)


def _centered_at(vel, c):
    """getCentered of cells c [m][3]; an upper face outside the grid (outermost layer: excluded by the contract) stays on the cell"""
    sz, sy, sx = vel.shape[:3]
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    out = np.zeros((len(c), 3), f32)
    out[:, 0] = f32(0.5) * (vel[z, y, x, 0] + vel[z, y, np.minimum(x + 1, sx - 1), 0])
    out[:, 1] = f32(0.5) * (vel[z, y, x, 1] + vel[z, np.minimum(y + 1, sy - 1), x, 1])
    if sz > 1:
        out[:, 2] = f32(0.5) * (vel[z, y, x, 2] + vel[np.minimum(z + 1, sz - 1), y, x, 2])
    return out


def _clipped(c, dims):
    return np.stack([np.clip(c[:, a], 0, dims[a] - 1) for a in range(3)], axis=1)


def cubic_velocity(flags, vel, x, c, radius, itype, counts=None):
    """sumNumerator / sumDenominator of the cubic mode, :351-368: itype cells around cell c of position x, x outer, z inner"""
    dims = _dims(flags)
    is3d = dims[2] > 1
    r = int(radius)
    rz = r if is3d else 0
    hs = f32(f32(r) * f32(1.732 if is3d else 1.414))
    sumN, sumD = np.zeros((len(x), 3), f32), np.zeros(len(x), f32)
    cnt = np.zeros(len(x), np.int64)
    with np.errstate(all="ignore"):
        for dx in range(-r, r + 1):
            for dy in range(-r, r + 1):
                for dz in range(-rz, rz + 1):
                    if dx == 0 and dy == 0 and dz == 0:
                        continue
                    q = c + np.array([dx, dy, dz])
                    qc = _clipped(q, dims)
                    ok = in_bounds(q, dims, 0) & ((flags[qc[:, 2], qc[:, 1], qc[:, 0]] & itype) != 0)
                    w = cubic_spline(hs, norm((x - q.astype(f32)).astype(f32)), 3 if is3d else 2)
                    cen = _centered_at(vel, qc)
                    sumN = np.where(ok[:, None], (sumN + (cen * w[:, None]).astype(f32)).astype(f32), sumN)
                    sumD = np.where(ok, (sumD + w).astype(f32), sumD)
                    cnt += ok
        if counts is not None:
            counts.append(cnt)
        return (sumN / sumD[:, None]).astype(f32)


def update_arrays(mode, pos, flag, v, l, f, flags, vel, ratio, radius, g, k_b, k_d, c_s, c_b, dt, exclude, antitunneling, itype,
                  info=None):
    """one knFlipUpdateSecondaryParticles{Linear,Cubic} pass; g is gravity / gridScale.  Returns pos, flag, v, l, kills"""
    pos, flag, v, l = np.array(pos, f32), np.array(flag, np.int32), np.array(v, f32), np.array(l, f32)
    flags, vel, ratio = np.asarray(flags, np.int32), np.asarray(vel, f32), np.asarray(ratio, f32)
    dims = _dims(flags)
    g, dt, k_b, k_d = np.asarray(g, f32), f32(dt), f32(k_b), f32(k_d)
    act = ((flag & PDELETE) == 0) & ((flag & exclude) == 0)
    c = to_int(pos)
    inb = in_bounds(c, dims, 0)
    out = act & ~inb
    flag[out] |= PDELETE
    kills = int(out.sum())
    idx = np.nonzero(act & inb)[0]
    ci, x, vv = c[idx], pos[idx], v[idx]
    with np.errstate(all="ignore"):
        nr = ratio[ci[:, 2], ci[:, 1], ci[:, 0]]
        spray = nr < f32(c_s)
        bubble = ~spray & (nr > f32(c_b))
        foam = ~spray & ~bubble
        typ = np.where(spray, PSPRAY, np.where(bubble, PBUBBLE, PFOAM)).astype(np.int32)
        fl = (flag[idx] | typ) & ~((PSPRAY | PBUBBLE | PFOAM) & ~typ)
        if mode == "cubic":
            counts = []
            uf = cubic_velocity(flags, vel, x, ci, radius, itype, counts)
            if info is not None:
                info["cubic_neighbours"] = np.where(~spray, counts[0], -1)
        else:
            uf = interp_mac(vel, x)
        v_s = (vv + (dt * (f[idx] + g).astype(f32)).astype(f32)).astype(f32)
        vj = ((uf - vv).astype(f32) / dt).astype(f32)
        v_b = (vv + (dt * ((k_b * -g).astype(f32) + (k_d * vj).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        vnew = np.where(spray[:, None], v_s, np.where(bubble[:, None], v_b, vv)).astype(f32)
        u = np.where(foam[:, None], uf, vnew).astype(f32)
        tun = np.zeros(len(idx), bool)
        first = np.zeros(len(idx), np.int64)
        for ct in range(1, int(antitunneling)):
            fct = f32(f32(f32(ct) * f32(f32(1) / f32(antitunneling))) * dt)
            t = to_int((x + (fct * u).astype(f32)).astype(f32))
            tc = _clipped(t, dims)
            hit = ~in_bounds(t, dims, 0) | ((flags[tc[:, 2], tc[:, 1], tc[:, 0]] & TypeObstacle) != 0)
            first = np.where(hit & ~tun, ct, first)
            tun |= hit
        xn = (x + (dt * u).astype(f32)).astype(f32)
        ln = (l[idx] - dt).astype(f32)
        dead = ~tun & (ln <= 0)
    v[idx] = vnew
    pos[idx] = np.where(tun[:, None], x, xn)
    l[idx] = np.where(tun, l[idx], ln)
    flag[idx] = np.where(tun | dead, fl | PDELETE, fl)
    kills += int(tun.sum() + dead.sum())
    if info is not None:
        info.update(idx=idx, type=typ, tunnel_ct=first, dead=dead, out=out)
    return pos, flag, v, l, kills


def do_compress(parts):
    """ParticleSystem::doCompress, particle.h:142-145"""
    if parts.deletes > parts.chunk:
        parts.compress_par()


def update(mode, parts, iv, il, i_f, flags, vel, ratio, radius, gravity, k_b, k_d, c_s, c_b, dt, scale_dx=None, exclude=PTRACER,
           antitunneling=0, itype=TypeFluid, info=None):
    """flipUpdateSecondaryParticles on a Parts: scale_dx is the solver's dx where `scale`, None otherwise"""
    g = (np.asarray(gravity, f32) / (f32(scale_dx) if scale_dx is not None else f32(1))).astype(f32)
    ch = parts.channels
    parts.pos, parts.flag, ch[iv].data, ch[il].data, kills = update_arrays(
        mode, parts.pos, parts.flag, ch[iv].data, ch[il].data, ch[i_f].data, flags, vel, ratio, radius, g, k_b, k_d, c_s, c_b, dt, exclude,
        antitunneling, itype, info)
    parts.deletes += kills
    do_compress(parts)
    return kills


def delete_in_obstacle(parts, flags):
    """flipDeleteParticlesInObstacle, :450-476"""
    flags = np.asarray(flags, np.int32)
    dims = _dims(flags)
    c = to_int(parts.pos)
    cc = _clipped(c, dims)
    act = (parts.flag & PDELETE) == 0
    hit = act & (~in_bounds(c, dims, 0) | ((flags[cc[:, 2], cc[:, 1], cc[:, 0]] & (TypeObstacle | TypeOutflow)) != 0))
    parts.flag = np.where(hit, parts.flag | PDELETE, parts.flag).astype(np.int32)
    parts.deletes += int(hit.sum())
    do_compress(parts)
    return int(hit.sum())


def set_flags_from_levelset(flags, phi, exclude=TypeObstacle, itype=TypeFluid):
    flags = np.asarray(flags, np.int32)
    return np.where((np.asarray(phi, f32) < 0) & ((flags & exclude) == 0), np.int32(itype), flags).astype(np.int32)


def set_mac_from_levelset(vel, phi, c):
    dims = _dims(phi)
    i, j, k = _cells(dims)
    corner = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(f32)
    on = (interp_real(np.asarray(phi, f32), corner) > 0).reshape(phi.shape)
    return np.where(on[..., None], np.asarray(c, f32), np.asarray(vel, f32)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs of the fixture cases (tests/golden/secparts.npz holds the reference's outputs only)
# ---------------------------------------------------------------------------------------------------------------------------------
def _shape(dims):
    return (dims[2], dims[1], dims[0])


def _interior(dims):
    """mask of the cells off the outermost layer (a 2-D grid has no z layer)"""
    m = np.zeros(_shape(dims), bool)
    m[(slice(1, -1) if dims[2] > 1 else slice(None)), 1:-1, 1:-1] = True
    return m


def _smooth(dims, rng, amp):
    sx, sy, sz = dims
    k, j, i = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    a = rng.uniform(0.3, 0.9, 3)
    p = rng.uniform(0, 6, 3)
    return (amp * (np.sin(a[0] * i + p[0]) + np.sin(a[1] * j + p[1]) + np.sin(a[2] * k + p[2]))).astype(f32)


# taus: (tauMinTA, tauMaxTA, tauMinWC, tauMaxWC, tauMinKE, tauMaxKE), about the 10th and 90th percentile of the case's raw sums, so
# that most potentials lie strictly inside (0, 1) and both clamps occur
POT_CASES = {
    "p3d_r1": dict(dims=(9, 8, 7), radius=1, seed=101, taus=(0.2, 4.5, 0.1, 2.5, 1.0, 20.0)),
    "p3d_r2": dict(dims=(9, 8, 7), radius=2, seed=102, taus=(11.0, 26.0, 4.5, 10.0, 3.0, 40.0)),
    "p3d_r3": dict(dims=(9, 8, 7), radius=3, seed=103, taus=(10.0, 50.0, 5.0, 40.0, 1.0, 10.0)),
    "p3d_row": dict(dims=(70, 6, 5), radius=2, seed=104, taus=(1.3, 3.3, 1.0, 10.0, 0.02, 0.4)),
    "p2d_r1": dict(dims=(33, 18, 1), radius=1, seed=105, taus=(0.1, 0.9, 0.05, 1.5, 0.05, 1.5)),
    "p2d_r2": dict(dims=(33, 18, 1), radius=2, seed=106, taus=(0.7, 2.2, 0.5, 7.0, 0.05, 1.5)),
    "p2d_thin_r1": dict(dims=(3, 50, 1), radius=1, seed=107, taus=(0.01, 0.15, 0.01, 0.1, 0.05, 0.8)),
    "p2d_thin_r2": dict(dims=(3, 50, 1), radius=2, seed=108, taus=(0.01, 0.15, 0.01, 0.1, 0.05, 0.8)),
    "p3d_types": dict(dims=(9, 8, 7), radius=1, seed=109, taus=(0.5, 3.3, 0.1, 1.8, 1.5, 25.0), itype=TypeEmpty, jtype=TypeObstacle | TypeFluid),
}


def pot_inputs(name, seed=None):
    """flags with about 15 % of each jtype kind, a fluid cell walled in by obstacles (0 / 0 neighbour ratio at radius 1), a block of
    zero velocity (getNormalized of 0) and a block where phi = x (a unit normal: the "normalized enough" branch)"""
    c = POT_CASES[name]
    dims = sx, sy, sz = c["dims"]
    rng = np.random.RandomState(c["seed"] if seed is None else seed)
    sh = _shape(dims)
    u = rng.uniform(size=sh)
    flags = np.where(u < 0.15, TypeObstacle, np.where(u < 0.30, TypeOutflow, np.where(u < 0.45, TypeInflow,
                     np.where(u < 0.85, TypeFluid, TypeEmpty)))).astype(np.int32)
    flags[~_interior(dims)] = TypeObstacle
    wz = sz // 2
    wy, wx = sy // 2, min(sx // 2, sx - 2)
    if sx >= 5:
        flags[max(wz - 1, 0):wz + 2, wy - 1:wy + 2, wx - 1:wx + 2] = TypeObstacle
        flags[wz, wy, wx] = TypeFluid
    vel = (rng.uniform(-1, 1, sh + (3,)) * 1.5).astype(f32)
    vel[:, 1:4, 1:4] = 0
    if sz == 1:
        vel[..., 2] = 0
    phi = (_smooth(dims, rng, 1.0) + rng.uniform(-0.2, 0.2, sh)).astype(f32)
    if sx >= 8:
        phi[:, -4:, 4:8] = np.arange(4, 8, dtype=f32)[None, None, :]
    normal = np.full(sh + (3,), 7.0, f32)
    return dict(dims=dims, flags=flags, vel=vel, phi=phi, normal=normal, radius=c["radius"], taus=c["taus"], scale=f32(1.0 / max(dims)) * f32(4),
                itype=c.get("itype", TypeFluid), jtype=c.get("jtype", JTYPE))


def run_pot_case(name):
    I = pot_inputs(name)
    ta, wc, ke, nr, normal = potentials(I["flags"], I["vel"], I["normal"], I["phi"], I["radius"], *I["taus"], I["scale"], I["itype"], I["jtype"])
    return dict(potTA=ta, potWC=wc, potKE=ke, ratio=nr, normal=normal)


# sampling: all cases of one mode run in this order in one process (the stream is process-wide)
SAMPLE_PAR = dict(lMin=2.0, lMax=5.0, c_s=0.3, c_b=0.7, k_ta=700.0, k_wc=-30.0, dt=0.5, solver_dt=0.5, peak=0.0, on_ta=0.01)
SAMPLE_CASES = {
    "s3d": dict(dims=(67, 9, 5), seed=201, peak=6.0), "s2d": dict(dims=(40, 30, 1), seed=202, peak=3.0, np0=0),
    "s3d_none": dict(dims=(67, 9, 5), seed=203, k_ta=0.0, k_wc=0.0),
    "s3d_twice": dict(dims=(67, 9, 5), seed=204, calls=2, dt=0.0, solver_dt=0.25, on_ta=0.08),
}
SAMPLE_ORDER = ("s3d", "s2d", "s3d_none", "s3d_twice")
MODES = ("single", "multiple")


def sec_system(rng, n, dims, pos=None):
    """a secondary system with channels v_sec, l_sec, f_sec and an extra int channel, built as the recorder builds it: through add(),
    so mDeleteChunk = n / 20 and mDeletes = 0; flags are set afterwards (deleted slots are not counted)"""
    if pos is None:
        pos = rng.uniform(1, np.array(dims) - 1, (n, 3))
    pos = np.asarray(pos, f32)
    if dims[2] == 1:
        pos[:, 2] = 0
    kinds = np.array([0, PSPRAY, PBUBBLE, PFOAM, PTRACER, PDELETE, PDELETE | PFOAM, PSPRAY | PBUBBLE], np.int32)
    flag = kinds[rng.randint(0, len(kinds), n)]
    ch = [Channel("vec3", rng.uniform(-2, 2, (n, 3))), Channel("real", rng.uniform(0.2, 3, n)), Channel("vec3", rng.uniform(-0.3, 0.3, (n, 3))),
          Channel("int", rng.randint(1, 1000, n))]
    return Parts(pos, flag, ch, 0, n // N.DELETE_PART)


def sample_inputs(name):
    """potentials: most cells emit nothing, a tenth a few, one cell (`peak`: its trapped-air value) more than 300 per entry in either
    mode, some cells a negative count (negative k_wc); non-fluid cells with potentials; a NaN neighbour ratio; a system with deleted
    slots and an extra channel"""
    c = dict(SAMPLE_PAR)
    c.update(SAMPLE_CASES[name])
    dims = sx, sy, sz = c["dims"]
    rng = np.random.RandomState(c["seed"])
    sh = _shape(dims)
    # blocks of 2x2(x2) cells with one value each (a lone cell's potentials, interpolated at the cylinders of "multiple", emit nothing)
    on = rng.uniform(size=sh) < 0.012
    KE = np.where(on, rng.uniform(0.3, 1, sh), 0).astype(f32)
    TA = np.where(on, rng.uniform(0, c["on_ta"], sh), 0).astype(f32)
    for ax in range(3):
        KE, TA = np.maximum(KE, np.roll(KE, 1, axis=ax)), np.maximum(TA, np.roll(TA, 1, axis=ax))
    WC = np.zeros(sh, f32)
    neg = rng.uniform(size=sh) < 0.02
    KE[neg], TA[neg], WC[neg] = 1.0, 0.0, 0.5
    z0 = 1 if sz > 1 else 0
    if c["peak"]:
        KE[z0 + 1 if sz > 1 else 0, 4, 10], TA[z0 + 1 if sz > 1 else 0, 4, 10], WC[z0 + 1 if sz > 1 else 0, 4, 10] = 1.0, c["peak"], 0.0
    flags = np.where(rng.uniform(size=sh) < 0.85, TypeFluid, TypeEmpty).astype(np.int32)
    flags[~_interior(dims)] = TypeObstacle
    flags[z0:z0 + 3, 3:6, 9:12] = TypeFluid
    vel = (rng.uniform(-1, 1, sh + (3,)) * 2.0).astype(f32)
    vel[:, 1:3, 1:5] = 0
    if sz == 1:
        vel[..., 2] = 0
    ratio = rng.uniform(0, 1, sh).astype(f32)
    ratio[z0 + 1 if sz > 1 else 0, 4, 10] = np.nan
    parts = sec_system(rng, c.get("np0", 40), dims)
    c.update(flags=flags, vel=vel, potTA=TA, potWC=WC, potKE=KE, ratio=ratio, parts=parts, calls=c.get("calls", 1))
    return c


def run_sample_case(mode, name, stream, serial=False):
    """the model's result of a sampling case: the system after the calls, the radii of the new particles and the reals drawn"""
    I = sample_inputs(name)
    P = I["parts"]
    dt = I["dt"] if I["dt"] > 0 else I["solver_dt"]
    radii, sizes, start = [], [], stream.cursor
    for _ in range(I["calls"]):
        new = (sample_serial if serial else sample_orderfree)(mode, I["flags"], I["vel"], I["potTA"], I["potWC"], I["potKE"], I["ratio"],
                                                              I["lMin"], I["lMax"], I["c_s"], I["c_b"], I["k_ta"], I["k_wc"], dt, stream)
        sample(P, 0, 1, new)
        radii.append(new["r"])
        sizes.append(P.size())
    return P, np.concatenate(radii), np.array(sizes, np.int64), stream.cursor - start


UPDATE_GRIDS = {"3d": (20, 16, 12), "2d": (24, 20, 1)}
UPDATE_PAR = dict(gravity=(0.0, -0.05, 0.01), k_b=0.6, k_d=0.4, c_s=0.3, c_b=0.7, solver_dt=0.5, exclude=PTRACER, itype=TypeFluid)
UPDATE_CASES = {
    "u_lin_1": dict(grid="3d", mode="linear", n=1, at=0, dt=0.5, scale=True, seed=301),
    "u_lin_63": dict(grid="2d", mode="linear", n=63, at=1, dt=0.5, scale=False, seed=302),
    "u_lin_64": dict(grid="3d", mode="linear", n=64, at=4, dt=0.5, scale=True, seed=303),
    "u_lin_65": dict(grid="2d", mode="linear", n=65, at=4, dt=0.0, scale=True, seed=304),
    "u_lin_1000": dict(grid="3d", mode="linear", n=1000, at=4, dt=0.0, scale=False, seed=305),
    "u_lin_5000": dict(grid="2d", mode="linear", n=5000, at=4, dt=0.5, scale=True, seed=306, fixture=False),
    "u_lin_calm": dict(grid="3d", mode="linear", n=1000, at=0, dt=0.5, scale=True, seed=307, calm=True),
    "u_cub_1": dict(grid="2d", mode="cubic", radius=1, n=1, at=0, dt=0.5, scale=True, seed=311),
    "u_cub_64": dict(grid="3d", mode="cubic", radius=1, n=64, at=1, dt=0.5, scale=False, seed=312),
    "u_cub_65": dict(grid="2d", mode="cubic", radius=2, n=65, at=4, dt=0.0, scale=True, seed=313),
    "u_cub_1000": dict(grid="3d", mode="cubic", radius=2, n=1000, at=4, dt=0.5, scale=True, seed=314),
    "u_cub_5000": dict(grid="2d", mode="cubic", radius=1, n=5000, at=4, dt=0.5, scale=False, seed=315, fixture=False),
    "u_cub_calm": dict(grid="2d", mode="cubic", radius=2, n=1000, at=0, dt=0.5, scale=True, seed=316, calm=True),
}
# fixture=False: a case the GPU test runs against this model only (the fixture file stays small)
DELETE_CASES = {"d3d": dict(grid="3d", n=1000, seed=401), "d2d": dict(grid="2d", n=1000, seed=402),
                "d3d_calm": dict(grid="3d", n=1000, seed=403, calm=True)}


def particle_grid(dims, rng, outflow=False):
    """fluid inside a wall layer, an obstacle block two cells thick, a few empty cells (and outflow cells for the delete cases)"""
    sx, sy, sz = dims
    flags = np.where(rng.uniform(size=_shape(dims)) < 0.9, TypeFluid, TypeEmpty).astype(np.int32)
    if outflow:
        flags[:, 2:5, -4:-1] = TypeOutflow | TypeEmpty
    flags[~_interior(dims)] = TypeObstacle
    flags[(slice(3, 8) if sz > 1 else slice(None)), 5:10, 8:10] = TypeObstacle
    return flags


def update_inputs(name, table=None):
    c = dict(UPDATE_PAR)
    c.update((table or UPDATE_CASES)[name])
    dims = UPDATE_GRIDS[c["grid"]]
    rng = np.random.RandomState(c["seed"])
    n, calm = c["n"], c.get("calm", False)
    flags = particle_grid(dims, rng, outflow=table is DELETE_CASES)
    sh = _shape(dims)
    vel = (rng.uniform(-1, 1, sh + (3,)) * (0.5 if calm else 6.0)).astype(f32)
    if dims[2] == 1:
        vel[..., 2] = 0
    ratio = rng.uniform(0, 1, sh).astype(f32)
    size = np.array(dims, f64)
    if calm:
        pos = rng.uniform(3, size - 3, (n, 3))
        pos[:, 0] = rng.uniform(11, dims[0] - 3, n)         # clear of the obstacle block
    else:
        pos = rng.uniform(-1.5, size + 0.5, (n, 3))
        if dims[2] == 1:
            pos[:, 2] = rng.uniform(-1.2, 1.2, n)
        if n >= 63:
            pos[5] = (-0.5, 3.3, 0.4)        # a coordinate in (-1, 0): cell 0
            pos[6] = (4.2, -0.25, 0.6)
            pos[7, 2] = -0.75 if dims[2] > 1 else 0.9
    parts = sec_system(rng, n, dims, pos)
    if calm:
        parts.flag = np.where(parts.flag & PDELETE, PFOAM, parts.flag).astype(np.int32)
        parts.channels[1].data = rng.uniform(2, 3, n).astype(f32)
        parts.channels[0].data = (parts.channels[0].data * f32(0.2)).astype(f32)
        few = rng.choice(n, max(n // 50, 1), replace=False)
        if table is DELETE_CASES:
            parts.pos[few, 0] = 8.5          # inside the obstacle block
            parts.pos[few, 1] = 6.5
            if dims[2] > 1:
                parts.pos[few, 2] = 4.5
    dt = c["dt"] if c.get("dt", 0) > 0 else c["solver_dt"]
    if not calm and n >= 63:
        parts.channels[1].data[10:14] = f32(dt)         # a lifetime that ends at exactly 0
    if calm and table is None:
        parts.channels[1].data[few] = f32(dt)           # a few kills, fewer than mDeleteChunk: doCompress leaves them in place
    c.update(dims=dims, flags=flags, vel=vel, ratio=ratio, parts=parts, step=dt, dx=1.0 / max(dims), radius=c.get("radius", 1))
    return c


def run_update_case(name, info=None):
    I = update_inputs(name)
    P = I["parts"]
    update(I["mode"], P, 0, 1, 2, I["flags"], I["vel"], I["ratio"], I["radius"], I["gravity"], I["k_b"], I["k_d"], I["c_s"], I["c_b"], I["step"],
           I["dx"] if I["scale"] else None, I["exclude"], I["at"], I["itype"], info)
    return P


def run_delete_case(name):
    I = update_inputs(name, DELETE_CASES)
    delete_in_obstacle(I["parts"], I["flags"])
    return I["parts"]


SET_CASES = {"f3d": dict(dims=(7, 5, 3), seed=501), "f2d": dict(dims=(33, 31, 1), seed=502)}


def set_inputs(name):
    c = SET_CASES[name]
    dims = c["dims"]
    rng = np.random.RandomState(c["seed"])
    sh = _shape(dims)
    kinds = np.array([TypeFluid, TypeObstacle, TypeEmpty, TypeOutflow | TypeEmpty, TypeObstacle | 64, TypeInflow], np.int32)
    return dict(dims=dims, flags=kinds[rng.randint(0, len(kinds), sh)], phi=rng.uniform(-1, 1, sh).astype(f32),
                vel=rng.uniform(-1, 1, sh + (3,)).astype(f32), c=(1.0, -2.0, 3.0), exclude=TypeObstacle, itype=TypeFluid)


def parts_state(P):
    d = {"pos": P.pos.copy(), "flag": P.flag.copy()}
    for q, c in enumerate(P.channels):
        d["ch%d" % q] = c.data.copy()
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorded loop: scenes/flip01_simple.py in 3-D at LOOP["res"]^3 with a secondary system beside it
# ---------------------------------------------------------------------------------------------------------------------------------
LOOP = dict(res=32, steps=12, dt=0.5, radius=2, taus=(2.0, 12.0, 1.0, 8.0, 0.02, 0.4), scale=4.0 / 32, lMin=1.0, lMax=4.0, c_s=0.4,
            c_b=0.8, k_ta=40.0, k_wc=40.0, k_b=0.5, k_d=0.4, gravity=(0.0, -0.004, 0.0), antitunneling=4)


def sec_loop(m, before=None, after=None):
    """the recorded loop in the package's API (GPU backend).  before(call, t, objects) / after(call, t, objects) run around each of
    the four secondary-particle calls ("potentials", "sample", "update", "delete").  Returns counts [steps][6] as the recorder
    stores them (live, spawned, slots, live spray / bubble / foam) and the four potential grids at the end."""
    C = LOOP
    res, steps = C["res"], C["steps"]
    gs = m.vec3(res, res, res)
    s = m.Solver(name="main", gridSize=gs, dim=3)
    s.timestep = C["dt"]
    flags, phi = s.create(m.FlagGrid), s.create(m.LevelsetGrid)
    vel, velOld, pressure, tmpVec3, normal = s.create(m.MACGrid), s.create(m.MACGrid), s.create(m.RealGrid), s.create(m.VecGrid), s.create(m.VecGrid)
    potTA, potWC, potKE, ratio = (s.create(m.RealGrid) for _ in range(4))
    pp = s.create(m.BasicParticleSystem)
    pVel = pp.create(m.PdataVec3)
    pindex, gpi = s.create(m.ParticleIndexSystem), s.create(m.IntGrid)
    sec = s.create(m.BasicParticleSystem)
    vSec, lSec, fSec = sec.create(m.PdataVec3), sec.create(m.PdataReal), sec.create(m.PdataVec3)
    flags.initDomain(boundaryWidth=0)
    fluidbox = m.Box(parent=s, p0=gs * m.vec3(0, 0, 0), p1=gs * m.vec3(0.4, 0.6, 1))
    phiInit = fluidbox.computeLevelset()
    flags.updateFromLevelset(phiInit)
    m.sampleFlagsWithParticles(flags=flags, parts=pp, discretization=2, randomness=0.2)
    O = dict(s=s, flags=flags, phi=phi, vel=vel, normal=normal, potTA=potTA, potWC=potWC, potKE=potKE, ratio=ratio, sec=sec,
             chans=[vSec, lSec, fSec])
    counts = np.zeros((steps, 6), np.int64)

    def around(call, t, fn):
        if before:
            before(call, t, O)
        fn()
        if after:
            after(call, t, O)

    for t in range(steps):
        pp.advectInGrid(flags=flags, vel=vel, integrationMode=m.IntRK4, deleteInObstacle=False)
        m.mapPartsToMAC(vel=vel, flags=flags, velOld=velOld, parts=pp, partVel=pVel, weight=tmpVec3)
        m.extrapolateMACFromWeight(vel=vel, distance=2, weight=tmpVec3)
        m.markFluidCells(parts=pp, flags=flags)
        m.gridParticleIndex(parts=pp, flags=flags, indexSys=pindex, index=gpi)
        m.unionParticleLevelset(pp, pindex, flags, gpi, phi)
        m.addGravity(flags=flags, vel=vel, gravity=(0, -0.002, 0))
        m.setWallBcs(flags=flags, vel=vel)
        m.solvePressure(flags=flags, vel=vel, pressure=pressure)
        m.setWallBcs(flags=flags, vel=vel)
        m.extrapolateMACSimple(flags=flags, vel=vel)
        m.flipVelocityUpdate(vel=vel, velOld=velOld, flags=flags, parts=pp, partVel=pVel, flipRatio=0.97)
        around("potentials", t, lambda: m.flipComputeSecondaryParticlePotentials(
            potTA, potWC, potKE, ratio, flags, vel, normal, phi, C["radius"], *C["taus"], C["scale"]))
        size0 = sec.pySize()
        around("sample", t, lambda: m.flipSampleSecondaryParticles(
            "single", flags, vel, sec, vSec, lSec, C["lMin"], C["lMax"], potTA, potWC, potKE, ratio, C["c_s"], C["c_b"], C["k_ta"], C["k_wc"]))
        spawned = sec.pySize() - size0
        around("update", t, lambda: m.flipUpdateSecondaryParticles(
            "linear", sec, vSec, lSec, fSec, flags, vel, ratio, 1, C["gravity"], C["k_b"], C["k_d"], C["c_s"], C["c_b"],
            antitunneling=C["antitunneling"]))
        around("delete", t, lambda: m.flipDeleteParticlesInObstacle(sec, flags))
        fl = sec.get_flags()
        live = (fl & PDELETE) == 0
        counts[t] = [live.sum(), spawned, len(fl)] + [int((live & ((fl & b) != 0)).sum()) for b in (PSPRAY, PBUBBLE, PFOAM)]
        s.step()
    return counts, np.stack([g.to_numpy() for g in (potTA, potWC, potKE, ratio)])
